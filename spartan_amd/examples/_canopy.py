"""The two tile bodies of the canopy clustering driver: backend.canopy / backend.pdf_label where the backend has them
(HipBackend: sp_canopy, sp_pdf_label), NumPy on host arrays otherwise -- the same arithmetic, operation for operation
in the arrays' dtype and in the kernels' stated order (include/spartan_hip_canopy.h), so a backend of plain NumPy tiles
produces the kernels' bytes.  Both paths refuse through tile_checks.check_canopy and check_pdf_label (the launchers and
the HipBackend methods call them too)."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray


def _d2(rows, point):
  """The squared distances of `rows` [m, d] to one `point` [d] in their dtype: one accumulator per row that starts at
  0 and takes (c_j - x_j) * (c_j - x_j) for j = 0, 1, ... in turn.  (For d < 8 NumPy's own .sum() has this order.)"""
  acc = np.zeros(rows.shape[0], rows.dtype)
  for j in range(rows.shape[1]):
    t = rows[:, j] - point[j]
    acc = acc + t * t
  return acc


def canopy_numpy(x, t1, t2, chains=1):
  """(centers [m, d], counts [m] int64, rows [m] int64) of the reference's sequential loop (canopy_clustering.py:33-65,
  without the `count > cf` filter) over x [n, d] of a float dtype T: chain c owns the rows floor(c n / chains) ..
  floor((c + 1) n / chains) - 1 and walks them in order.  For every canopy so far, in creation order, d2 = the squared
  distance to its CREATING row (_d2); d2 < T(t1): count += 1, sum = sum + row; d2 < T(t2) for any: the row is bound; a
  row that is not bound becomes a canopy (count 1, sum = the row).  centers = sum / T(count); rows are the creating
  rows' indices in x.  All canopies of all chains, in chain order then creation order.  x is not written."""
  dt = x.dtype
  n, d = x.shape
  a1, a2 = dt.type(t1), dt.type(t2)
  out_c, out_n, out_r = [np.zeros((0, d), dt)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
  with np.errstate(all='ignore'):
    for c in range(chains):
      lo, hi = c * n // chains, (c + 1) * n // chains
      made = np.empty((max(hi - lo, 1), d), dt)           # the creating rows
      sums = np.empty((max(hi - lo, 1), d), dt)
      counts, rows, m = np.zeros(max(hi - lo, 1), np.int64), np.zeros(max(hi - lo, 1), np.int64), 0
      for i in range(lo, hi):
        point = x[i]
        dist = _d2(made[:m], point)
        seen = dist < a1
        counts[:m][seen] += 1
        sums[:m][seen] = sums[:m][seen] + point
        if not (dist < a2).any():
          made[m], sums[m], counts[m], rows[m] = point, point, 1, i
          m += 1
      out_c.append(sums[:m] / counts[:m].astype(dt)[:, None])
      out_n.append(counts[:m])
      out_r.append(rows[:m])
  centers = np.concatenate(out_c)
  assert centers.dtype == dt
  return centers, np.concatenate(out_n), np.concatenate(out_r)


def pdf_label_numpy(x, centers):
  """labels [n] int32 of the reference's _cluster_mapper (canopy_clustering.py:68-92): per row the lowest j at which
  pdf = 1 / (1 + d2_j) -- one add, one division in the arrays' dtype, d2 as _d2 -- is largest: strict <, starting from
  -1, so a NaN pdf never wins and no centre gives -1."""
  dt = x.dtype
  n = x.shape[0]
  one = dt.type(1)
  best, labels = np.full(n, -1, dt), np.full(n, -1, np.int32)
  with np.errstate(all='ignore'):
    for j in range(centers.shape[0]):
      pdf = one / (one + _d2(x, centers[j]))
      win = best < pdf
      best[win], labels[win] = pdf[win], j
  assert best.dtype == dt
  return labels


def canopy(x, t1, t2, chains=1, cap=None):
  """(centers [m, d], counts [m], rows [m]) of a row tile `x` [n, d], float32 or float64, as host arrays: all canopies
  of all chains, unfiltered (see canopy_numpy).  With an operand that lives on another rank the three are placeholders
  of no canopies: the size of the result depends on the data.  TypeError ("astype first") for other dtypes, ValueError
  for an x that is not 2-D, d < 1, chains < 1, cap < 1 and thresholds that are not finite."""
  if isinstance(x, distarray.Absent):
    dt, _, d, _, _, _, _, _ = tile_checks.check_canopy(x.dtype, x.shape, t1, t2, chains, cap)
    return distarray.Absent((0, d), dt), distarray.Absent((0,), np.int64), distarray.Absent((0,), np.int64)
  be = context.get().backend
  fn = getattr(be, 'canopy', None)
  if fn is not None:
    return fn(x, t1, t2, chains=chains, cap=cap)
  host = np.asarray(be.to_numpy(x))
  _, _, _, t1, t2, chains, _, _ = tile_checks.check_canopy(host.dtype, host.shape, t1, t2, chains, cap)
  return canopy_numpy(host, t1, t2, chains)


def pdf_label(x, centers):
  """The labels [n] int32 of a row tile `x` [n, d] among `centers` [k, d] as a new tile (see pdf_label_numpy).
  TypeError ("astype first") for other or mixed dtypes, ValueError for operands that are not 2-D, feature counts that
  differ and d < 1."""
  operands = (x, centers)
  if any(isinstance(t, distarray.Absent) for t in operands):
    _, n, _, _ = tile_checks.check_pdf_label([t.dtype for t in operands], [t.shape for t in operands])
    return distarray.Absent((n,), np.int32)
  be = context.get().backend
  fn = getattr(be, 'pdf_label', None)
  if fn is not None:
    return fn(x, centers)
  host = [np.asarray(be.to_numpy(t)) for t in operands]
  tile_checks.check_pdf_label([t.dtype for t in host], [t.shape for t in host])
  return pdf_label_numpy(*host)
