"""The tile bodies of the spectral-clustering driver: backend.affinity_degree / affinity_matrix where the backend has
them (HipBackend: sp_affinity_degree, sp_affinity_matrix), NumPy on host arrays otherwise -- the same recipe in the
tile's dtype (include/spartan_hip_spectral.h), which keeps the driver runnable on a backend of plain NumPy tiles."""
import numpy as np

from .. import _hip, context, tile_checks
from ..array import distarray

METRICS = tuple(_hip.SP_AFF_METRICS)


def check_params(metric, gamma, what='affinity'):
  """gamma as a float, or what sp_affinity_* refuses (tile_checks.check_affinity_params: NotImplementedError for
  'scaled_euclidean', ValueError for an unknown metric or a gamma that is not finite)."""
  return tile_checks.check_affinity_params(metric, gamma, what)[1]


def distance_numpy(x, y, metric):
  """d2 [m, n] (d1 for 'manhattan') in the dtype of x [m, d] and y [n, d], as the kernel forms it: (x - y)^2 (or
  |x - y|) added feature by feature onto 0, rounded after every operation."""
  dist = np.zeros((x.shape[0], y.shape[0]), x.dtype)
  with np.errstate(all='ignore'):
    for f in range(x.shape[1]):
      t = x[:, f:f + 1] - y[:, f][None, :]
      dist = dist + (np.abs(t) if metric == 'manhattan' else t * t)
  return dist


def affinity_numpy(x, y, metric, gamma):
  """a [m, n] in the dtype of x and y: exp(-(T(gamma) * d2)), sqrt(d2) or d1 of distance_numpy."""
  dt = x.dtype
  dist = distance_numpy(x, y, metric)
  with np.errstate(all='ignore'):
    if metric == 'rbf':
      a = np.exp(-(dt.type(gamma) * dist))
    else:
      a = np.sqrt(dist) if metric == 'euclidean' else dist
  assert a.dtype == dt
  return a


def degree_numpy(x, y, metric, gamma):
  """D [m]: the rows' sums of affinity_numpy.  The sum of a row is NumPy's (pairwise, over that row alone), in another
  order than the kernel's; like the kernel's it does not depend on the band the row is computed in."""
  a = np.ascontiguousarray(affinity_numpy(x, y, metric, gamma))
  return a.sum(axis=1) if a.shape[1] else np.zeros((a.shape[0],), a.dtype)


def matrix_numpy(x, r0, y, metric, gamma, scale=None):
  """out [m, n]: affinity_numpy, and with `scale` a_ij * (scale[r0 + i] * scale[j]) with exactly 1 at j = r0 + i."""
  a = affinity_numpy(x, y, metric, gamma)
  if scale is None:
    return a
  m = x.shape[0]
  out = a * (scale[r0:r0 + m, None] * scale[None, :])
  out[np.arange(m), r0 + np.arange(m)] = 1
  assert out.dtype == a.dtype
  return out


def _host_operands(be, *tiles):
  return [np.asarray(be.to_numpy(t)) for t in tiles if t is not None]


def affinity_degree(x, y, metric='rbf', gamma=1.0):
  """D [m] as a new tile: the sums over ALL rows of `y` [n, d] of the affinities of the rows of `x` [m, d]; both
  float32 or both float64."""
  if isinstance(x, distarray.Absent) or isinstance(y, distarray.Absent):
    return distarray.Absent((x.shape[0],), np.dtype(x.dtype))
  be = context.get().backend
  fn = getattr(be, 'affinity_degree', None)
  if fn is not None:
    return fn(x, y, metric, gamma)
  xh, yh = _host_operands(be, x, y)
  gamma = tile_checks.check_affinity_degree((xh.dtype, yh.dtype), (xh.shape, yh.shape), metric, gamma)[5]
  return degree_numpy(xh, yh, metric, gamma)


def affinity_matrix(x, r0, y, metric='rbf', gamma=1.0, scale=None):
  """out [m, n] as a new tile: the affinities of the rows of `x` -- points r0 .. r0 + m - 1 of `y` -- against all rows
  of `y`; with `scale` [n] the normalised matrix with a diagonal of exactly 1."""
  if isinstance(x, distarray.Absent) or isinstance(y, distarray.Absent):
    return distarray.Absent((x.shape[0], y.shape[0]), np.dtype(x.dtype))
  be = context.get().backend
  fn = getattr(be, 'affinity_matrix', None)
  if fn is not None:
    return fn(x, r0, y, metric, gamma, scale=scale)
  host = _host_operands(be, x, y, scale)
  gamma, r0 = tile_checks.check_affinity_matrix([t.dtype for t in host], [t.shape for t in host], r0, metric, gamma)[5:]
  return matrix_numpy(host[0], r0, host[1], metric, gamma, None if scale is None else host[2])
