"""The tile body of the fuzzy k-means driver: backend.fuzzy_step where the backend has it (HipBackend: sp_fuzzy_step),
NumPy on host arrays otherwise -- the same recipe in the tile's dtype (include/spartan_hip_fuzzy.h), which keeps the
driver runnable on a backend of plain NumPy tiles."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray

check_m = tile_checks.check_fuzzy_m      # (the driver checks its own m with it)


def step_numpy(x, c, m, want_u=False):
  """(labels int64 [n], sums [k, d], wsum [k]) and u [n, k] if wanted, in the dtype of x and c.  The distance is the
  kernel's: (x - c)^2 added feature by feature, rounded after every operation; the label is the first arg-max of d2
  (a NaN counts as the maximum).  The sums over centres and rows are NumPy's, in another order than the kernel's."""
  dt = x.dtype
  n, d = x.shape
  k = c.shape[0]
  with np.errstate(all='ignore'):
    d2 = np.zeros((n, k), dt)
    for f in range(d):
      t = x[:, f:f + 1] - c[:, f][None, :]
      d2 = d2 + t * t
    labels = np.argmax(d2, axis=1).astype(np.int64) if n else np.zeros((0,), np.int64)
    dist = np.sqrt(d2)
    dist[dist == 0] = dt.type(1e-10)
    p = dist if m == 2.0 else np.power(dist, dt.type(1.0 / (m - 1.0)))
    u = p / p.sum(axis=1)[:, None]
    w = u * u if m == 2.0 else np.power(u, dt.type(m))
    sums, wsum = w.T.dot(x), w.sum(axis=0)
  assert u.dtype == dt and sums.dtype == dt and wsum.dtype == dt
  return (labels, sums, wsum, u) if want_u else (labels, sums, wsum)


def fuzzy_step(points, centers, m, want_u=False):
  """One iteration on a row tile as new tiles: (labels int64 [n], sums [k, d], wsum [k]), plus u [n, k] when `want_u`
  is set; `points` [n, d] and `centers` [k, d] both float32 or both float64."""
  if isinstance(points, distarray.Absent) or isinstance(centers, distarray.Absent):
    n, k, d, dt = points.shape[0], centers.shape[0], points.shape[1], np.dtype(points.dtype)
    out = (distarray.Absent((n,), np.dtype(np.int64)), distarray.Absent((k, d), dt), distarray.Absent((k,), dt))
    return out + (distarray.Absent((n, k), dt),) if want_u else out
  be = context.get().backend
  fn = getattr(be, 'fuzzy_step', None)
  if fn is not None:
    return fn(points, centers, m, want_u=want_u)
  x, c = np.asarray(be.to_numpy(points)), np.asarray(be.to_numpy(centers))
  m = tile_checks.check_fuzzy_step((x.dtype, c.dtype), (x.shape, c.shape), m)[4]
  return step_numpy(x, c, m, want_u=want_u)
