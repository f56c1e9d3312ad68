"""The tile body of the ALS driver: backend.als_solve where the backend has it (HipBackend: sp_als_solve), NumPy on
host arrays otherwise -- the same normal equations, Cholesky and two triangular solves in the tile's dtype, which keeps
the driver runnable on a backend of plain NumPy tiles."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray


def _solve_rows(r, y, la, alpha, implicit):
  """(x [m, f], 1 + the lowest failing row or 0) in the dtype of r and y; a failing row of x is NaN."""
  from scipy.linalg import solve_triangular
  dt = r.dtype
  m, f = r.shape[0], y.shape[1]
  la, alpha = dt.type(la), dt.type(alpha)
  eye = np.eye(f, dtype=dt)
  x = np.zeros((m, f), dt)
  failed = 0
  gram = y.T.dot(y) if implicit else None
  with np.errstate(all='ignore'):
    for i in range(m):
      rated = r[i] != 0                          # (true for NaN: the row then fails below)
      ri, ys = r[i][rated], y[rated]
      if implicit:
        a = (gram + (ys.T * (alpha * ri)).dot(ys)) + la * eye
        b = ys.T.dot(np.where(ri > 0, 1 + alpha * ri, 0).astype(dt))
      else:
        if not ri.size:
          continue                               # nothing rated: exactly 0, the reference's lstsq of a zero system
        a = ys.T.dot(ys) + (la * dt.type(ri.size)) * eye
        b = ys.T.dot(ri)
      low = None
      if np.all(np.isfinite(a)) and np.all(np.isfinite(b)):
        try:
          low = np.linalg.cholesky(a)
        except np.linalg.LinAlgError:
          low = None
      if low is None or not np.all(np.diagonal(low) > 0):
        x[i] = np.nan
        failed = failed or i + 1
        continue
      z = solve_triangular(low, b, lower=True, check_finite=False)
      x[i] = solve_triangular(low.T, z, lower=False, check_finite=False)
  assert x.dtype == dt
  return x, failed


def als_solve(ratings, factors, la, alpha, implicit, info=None):
  """One half-step as a new [m, f] tile: row i solves its normal equations built from row i of `ratings` [m, n] and
  `factors` [n, f], both float32 or both float64 (include/spartan_hip_als.h states the two modes).  `info`: a one-
  element int32 tile of the backend, zero before the first solve that shares it; it receives 1 + the lowest failing
  row if it is still 0, and that row of the result is NaN."""
  if isinstance(ratings, distarray.Absent) or isinstance(factors, distarray.Absent):
    return distarray.Absent((ratings.shape[0], factors.shape[1]), factors.dtype)
  be = context.get().backend
  fn = getattr(be, 'als_solve', None)
  if fn is not None:
    return fn(ratings, factors, la, alpha, implicit=implicit, info=info)
  r, y = np.asarray(be.to_numpy(ratings)), np.asarray(be.to_numpy(factors))
  tile_checks.check_als_solve((r.dtype, y.dtype), (r.shape, y.shape))
  x, failed = _solve_rows(r, y, la, alpha, bool(implicit))
  if failed and info is not None and not info[0]:
    info[0] = failed
  return x
