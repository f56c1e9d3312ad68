"""The tile bodies of the nearest-neighbour driver: backend.knn / backend.knn_merge where the backend has them
(HipBackend: sp_knn / sp_knn_merge), NumPy on host arrays otherwise -- the same arithmetic and the same order, which
keeps the driver runnable on a backend of plain NumPy tiles."""
import numpy as np

from .... import context, tile_checks
from ....array import distarray
from ..._select import select


def _absent_pair(nq, k, dtype):
  return distarray.Absent((nq, k), dtype), distarray.Absent((nq, k), np.int64)


def knn(queries, points, k, index_offset=0):
  """(dist2, idx), both [nq, k]: the k rows of the tile `points` nearest to every row of `queries` by the squared
  Euclidean distance sum_j (q_j - x_j)^2 in the tiles' dtype, ascending by (distance, index), idx = index_offset + row;
  +inf / -1 where the tile has fewer than k rows."""
  if isinstance(queries, distarray.Absent) or isinstance(points, distarray.Absent):
    return _absent_pair(queries.shape[0], k, points.dtype)
  be = context.get().backend
  fn = getattr(be, 'knn', None)
  if fn is not None:
    return fn(queries, points, k, index_offset=index_offset)
  q, x = np.asarray(be.to_numpy(queries)), np.asarray(be.to_numpy(points))
  k = tile_checks.check_knn((q.dtype, x.dtype), (q.shape, x.shape), k)[4]
  d2 = np.zeros((q.shape[0], x.shape[0]), q.dtype)
  with np.errstate(all='ignore'):
    for j in range(q.shape[1]):            # (one feature after the other onto one accumulator, as the kernel adds them)
      diff = q[:, j, None] - x[None, :, j]
      d2 = d2 + diff * diff
  idx = np.broadcast_to(np.arange(x.shape[0], dtype=np.int64) + int(index_offset), d2.shape)
  return select(d2, idx, ~np.isnan(d2), k)


def knn_merge(cand_dist2, cand_idx, k):
  """(dist2, idx), both [nq, k]: per row the k smallest by (distance, index) of the candidates; those with a negative
  index are padding."""
  if isinstance(cand_dist2, distarray.Absent) or isinstance(cand_idx, distarray.Absent):
    return _absent_pair(cand_dist2.shape[0], k, cand_dist2.dtype)
  be = context.get().backend
  fn = getattr(be, 'knn_merge', None)
  if fn is not None:
    return fn(cand_dist2, cand_idx, k)
  d2, idx = np.asarray(be.to_numpy(cand_dist2)), np.asarray(be.to_numpy(cand_idx))
  k = tile_checks.check_knn_merge((d2.dtype, idx.dtype), (d2.shape, idx.shape), k)[3]
  return select(d2, idx, (idx >= 0) & ~np.isnan(d2), k)
