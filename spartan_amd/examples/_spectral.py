"""The tile bodies of the spectral-clustering driver: backend.affinity_degree / affinity_matrix where the backend has
them (HipBackend: sp_affinity_degree, sp_affinity_matrix), NumPy on host arrays otherwise -- the same recipe in the
tile's dtype (include/spartan_hip_spectral.h), which keeps the driver runnable on a backend of plain NumPy tiles."""
import numpy as np

from .. import _hip, context
from ..array import distarray

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
METRICS = tuple(_hip.SP_AFF_METRICS)


def check_params(metric, gamma, what='affinity'):
  """gamma as a float, or what sp_affinity_* refuses (_hip.check_affinity_params: NotImplementedError for
  'scaled_euclidean', ValueError for an unknown metric or a gamma that is not finite)."""
  return _hip.check_affinity_params(metric, gamma, what)[1]


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


def _host_operands(what, be, x, y, scale=None):
  xh, yh = np.asarray(be.to_numpy(x)), np.asarray(be.to_numpy(y))
  sh = None if scale is None else np.asarray(be.to_numpy(scale))
  for t in (xh, yh, sh):
    if t is not None and t.dtype not in _FLOATS:
      raise TypeError('%s: dtype %s is not supported (float32 float64); convert with astype first' % (what, t.dtype))
  for t in (yh, sh):
    if t is not None and t.dtype != xh.dtype:
      raise TypeError('%s: operands of two dtypes (%s, %s); convert with astype first' % (what, xh.dtype, t.dtype))
  if xh.ndim != 2 or yh.ndim != 2 or xh.shape[1] != yh.shape[1]:
    raise ValueError('%s: shapes %s and %s do not fit' % (what, xh.shape, yh.shape))
  return xh, yh, sh


def affinity_degree(x, y, metric='rbf', gamma=1.0):
  """D [m] as a new tile: the sums over ALL rows of `y` [n, d] of the affinities of the rows of `x` [m, d]; both
  float32 or both float64."""
  if isinstance(x, distarray.Absent) or isinstance(y, distarray.Absent):
    return distarray.Absent((x.shape[0],), np.dtype(x.dtype))
  be = context.get().backend
  fn = getattr(be, 'affinity_degree', None)
  if fn is not None:
    return fn(x, y, metric, gamma)
  xh, yh, _ = _host_operands('affinity_degree', be, x, y)
  return degree_numpy(xh, yh, metric, check_params(metric, gamma, 'affinity_degree'))


def affinity_matrix(x, r0, y, metric='rbf', gamma=1.0, scale=None):
  """out [m, n] as a new tile: the affinities of the rows of `x` -- points r0 .. r0 + m - 1 of `y` -- against all rows
  of `y`; with `scale` [n] the normalised matrix with a diagonal of exactly 1."""
  if isinstance(x, distarray.Absent) or isinstance(y, distarray.Absent):
    return distarray.Absent((x.shape[0], y.shape[0]), np.dtype(x.dtype))
  be = context.get().backend
  fn = getattr(be, 'affinity_matrix', None)
  if fn is not None:
    return fn(x, r0, y, metric, gamma, scale=scale)
  xh, yh, sh = _host_operands('affinity_matrix', be, x, y, scale)
  gamma = check_params(metric, gamma, 'affinity_matrix')
  r0 = int(r0)
  if r0 < 0 or r0 + xh.shape[0] > yh.shape[0]:
    raise ValueError('affinity_matrix: rows %d .. %d are not among the %d points' % (r0, r0 + xh.shape[0], yh.shape[0]))
  if sh is not None and sh.shape != (yh.shape[0],):
    raise ValueError('affinity_matrix: a scale of shape %s for %d points' % (sh.shape, yh.shape[0]))
  return matrix_numpy(xh, r0, yh, metric, gamma, sh)
