"""The tile body of the linear SVM driver: backend.svm_dca where the backend has it (HipBackend: sp_svm_dca), NumPy on
host arrays otherwise -- the same arithmetic, operation for operation in the arrays' dtype and with the kernel's order
of the two inner products (include/spartan_hip_svm.h), so a backend of plain NumPy tiles produces the kernel's bits.
Both paths refuse through one function, tile_checks.check_svm_dca (the launcher and HipBackend.svm_dca call it too)."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray

check_operands = tile_checks.check_svm_dca


def lane_dot(p, r):
  """dot(p, r) of two [rows, 64 K] arrays (or two [64 K] vectors) as the kernel forms it: lane l of 64 starts at +0 and
  adds p_j * r_j for j = l, l + 64, ... in ascending order; the 64 lane sums are added as a balanced tree, partners at
  distance 32 first, then 16, 8, 4, 2 and 1.  Columns past d hold zeros in both and add +0."""
  prod = p * r
  prod = prod.reshape(prod.shape[:-1] + (prod.shape[-1] // 64, 64))
  acc = np.zeros(prod.shape[:-2] + (64,), prod.dtype)
  for k in range(prod.shape[-2]):
    acc = acc + prod[..., k, :]
  for s in (32, 16, 8, 4, 2, 1):
    acc = acc[..., :s] + acc[..., s:2 * s]
  return acc[..., 0]


def dca_numpy(x, y, alpha, w0, scaled_lambda, chains=1):
  """(alpha' [m, 1], w [chains, d]) of one pass over x [m, d] with y and alpha ([m] or [m, 1]) from w0 ([d] or [d, 1]),
  all of one float dtype T: chain c owns the rows floor(c m / chains) .. floor((c + 1) m / chains) - 1, starts from w0
  and per row, every operation rounded once in T,
      A = s dot(x, x)    B = dot(x, w)    g = (y - B) / A    v = y (g + a)    c = max(0, min(1, v)) as Python has them
      dl = y c - a       w = w + (x s) dl       a' = a + dl
  with s = T(scaled_lambda) and lane_dot's order.  No operand is written."""
  dt = x.dtype
  m, d = x.shape
  y, alpha, w0 = y.reshape(m), alpha.reshape(m), w0.reshape(d)
  s, one, zero = dt.type(scaled_lambda), dt.type(1), dt.type(0)
  pad = -(-d // 64) * 64
  xp = np.zeros((m, pad), dt)
  xp[:, :d] = x
  out, w_out = np.array(alpha, dt), np.empty((chains, d), dt)
  with np.errstate(all='ignore'):
    a_all = s * lane_dot(xp, xp)
    xs = x * s
    for c in range(chains):
      wp = np.zeros((pad,), dt)
      wp[:d] = w0
      for i in range(c * m // chains, (c + 1) * m // chains):
        yi, ai = y[i], alpha[i]
        g = (yi - lane_dot(xp[i], wp)) / a_all[i]
        v = yi * (g + ai)
        c1 = v if v < one else one
        c2 = c1 if c1 > zero else zero
        dl = yi * c2 - ai
        wp[:d] = wp[:d] + xs[i] * dl
        out[i] = ai + dl
      w_out[c] = wp[:d]
  assert out.dtype == dt and a_all.dtype == dt and xs.dtype == dt
  return out.reshape(m, 1), w_out


def svm_dca(x, y, alpha, w0, scaled_lambda, chains=1, want_w=False):
  """The new alpha [m, 1] of a row tile as a new tile, or (alpha, w [chains, d]) with `want_w`; `x` [m, d], `y` and
  `alpha` [m] or [m, 1], `w0` [d] or [d, 1], all float32 or all float64.  TypeError ("astype first") for other or mixed
  dtypes, ValueError for shapes that do not fit, d outside 1 .. 4096, chains < 1 and a scaled_lambda that is not
  finite and > 0."""
  operands = (x, y, alpha, w0)
  if any(isinstance(t, distarray.Absent) for t in operands):
    dt, m, d, _, chains = check_operands([t.dtype for t in operands], [t.shape for t in operands], scaled_lambda, chains)
    out = distarray.Absent((m, 1), dt)
    return (out, distarray.Absent((chains, d), dt)) if want_w else out
  be = context.get().backend
  fn = getattr(be, 'svm_dca', None)
  if fn is not None:
    return fn(x, y, alpha, w0, scaled_lambda, chains=chains, want_w=want_w)
  host = [np.asarray(be.to_numpy(t)) for t in operands]
  _, _, _, scaled_lambda, chains = check_operands([t.dtype for t in host], [t.shape for t in host], scaled_lambda, chains)
  out, w = dca_numpy(*host, scaled_lambda, chains)
  return (out, w) if want_w else out
