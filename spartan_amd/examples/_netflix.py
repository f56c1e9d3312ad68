"""The tile body of the Netflix SGD driver: backend.sgd_mf where the backend has it (HipBackend: sp_sgd_mf), NumPy on
host arrays otherwise -- the same sequence, operation for operation in the arrays' dtype and with the kernel's order of
the inner product (include/spartan_hip_mf.h), so a backend of plain NumPy tiles produces the kernel's bits.  Both paths
refuse through one function, tile_checks.check_sgd_mf (the launcher and HipBackend.sgd_mf call it too)."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray

check_operands = tile_checks.check_sgd_mf


def lanes_of(f):
  """L of include/spartan_hip_mf.h: the lanes that share a rating's inner product; a function of f alone."""
  return 8 if f <= 16 else (16 if f <= 64 else 64)


def lane_dot(p, q):
  """dot(p, q) of two [f] vectors as the kernel forms it: lane l of L = lanes_of(f) starts at +0 and adds p_k * q_k
  for k = l, l + L, ... in ascending order (a lane without a k keeps +0); the L lane sums are added as a balanced tree,
  partners at distance L / 2 first."""
  f = p.shape[0]
  lanes = lanes_of(f)
  prod = p * q
  acc = np.zeros(lanes, prod.dtype)
  for k in range(0, f, lanes):
    w = min(lanes, f - k)
    acc[:w] = acc[:w] + prod[k:k + w]
  s = lanes // 2
  while s >= 1:
    acc = acc[:s] + acc[s:2 * s]
    s //= 2
  return acc[0]


def sgd_numpy(indptr, indices, vals, u, m, lr, abs_err=None):
  """The sequence over a tile in canonical CSR, every operation rounded once in the arrays' dtype T: for each stored
  entry (i, j, r), rows ascending and columns ascending inside a row,
      d = r - lane_dot(u_i, m_j)      u_i = u_i + (u_i * d) * lr      m_j = m_j + (m_j * d) * lr      lr = T(lr)
  `u` and `m` are updated IN PLACE; abs_err[e] <- |d| where given."""
  dt = u.dtype
  lr = dt.type(lr)
  with np.errstate(all='ignore'):
    for i in range(len(indptr) - 1):
      for e in range(int(indptr[i]), int(indptr[i + 1])):
        j = int(indices[e])
        ui, mj = u[i], m[j]
        d = vals[e] - lane_dot(ui, mj)
        u[i] = ui + (ui * d) * lr
        m[j] = mj + (mj * d) * lr
        if abs_err is not None:
          abs_err[e] = np.abs(d)
  assert u.dtype == dt and m.dtype == dt


def sgd_mf(v, u, m, lr=None, want_error=False):
  """One pass over the stored entries of the sparse tile `v` [rows, cols], updating `u` [rows, f] and `m` [cols, f]
  (float32 or float64 like v's values) IN PLACE.  Returns None, or with `want_error` the sum of |d| over the tile's
  entries as a new [1, 1] tile (HipBackend: summed by the reduce kernel).  TypeError ("astype first") for other or mixed
  dtypes, ValueError for shapes that do not fit, f outside 1 .. 512 and an lr that is not finite.  Where an operand is
  Absent (another rank runs this tile) nothing is computed."""
  operands = (v, u, m)
  if any(isinstance(t, distarray.Absent) for t in operands):
    dt = check_operands([t.dtype for t in operands], v.shape, u.shape, m.shape, lr)[0]
    return distarray.Absent((1, 1), dt) if want_error else None
  be = context.get().backend
  fn = getattr(be, 'sgd_mf', None)
  if fn is not None:
    err = fn(v, u, m, lr=lr, want_error=want_error)
    if not want_error:
      return None
    return err.sum().reshape((1, 1)) if err.numel() else be.zeros((1, 1), be.dtype_of(u))
  indptr, indices, vals = (np.asarray(t) for t in be.sparse_parts(v))
  dt, _, _, _, lr = check_operands([vals.dtype, u.dtype, m.dtype], v.shape, u.shape, m.shape, lr)
  if not (isinstance(u, np.ndarray) and isinstance(m, np.ndarray)):
    raise TypeError('sgd_mf: U and M are updated in place: host arrays, got %s, %s' % (type(u).__name__, type(m).__name__))
  abs_err = np.zeros(len(indices), dt) if want_error else None
  sgd_numpy(indptr, indices, vals, u, m, lr, abs_err)
  return abs_err.sum(dtype=dt).reshape(1, 1) if want_error else None
