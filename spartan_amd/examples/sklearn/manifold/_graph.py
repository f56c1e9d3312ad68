"""The graph bodies of the Isomap driver: backend.graph_from_knn / backend.apsp where the backend has them (HipBackend:
sp_graph_from_knn / sp_apsp), NumPy on host arrays otherwise -- the same arithmetic (a candidate d[i][k] + d[k][j], one
rounded add, wins only if it is smaller), which keeps the driver runnable on a backend of plain NumPy tiles."""
import numpy as np

from .... import context, tile_checks


def graph_from_knn(dist, idx):
  """The dense undirected graph [n, n] of the neighbour lists dist (>= 0) and idx (int64), both [n, k]: +inf, 0 on the
  diagonal, and for every listed pair the smallest weight stated for it in either direction, on both sides.  idx < 0 is
  padding; idx >= n and idx = the row itself are skipped."""
  be = context.get().backend
  fn = getattr(be, 'graph_from_knn', None)
  if fn is not None:
    return fn(dist, idx)
  return graph_from_knn_numpy(np.asarray(be.to_numpy(dist)), np.asarray(be.to_numpy(idx)))


def graph_from_knn_numpy(dist, idx):
  """graph_from_knn on host arrays."""
  _, n, _ = tile_checks.check_graph_from_knn((dist.dtype, idx.dtype), (dist.shape, idx.shape))
  w = np.full((n, n), np.inf, dist.dtype)
  np.fill_diagonal(w, 0)
  rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], idx.shape)
  valid = (idx >= 0) & (idx < n) & (idx != rows)
  i, j, d = rows[valid], idx[valid], dist[valid]
  np.minimum.at(w, (i, j), d)
  np.minimum.at(w, (j, i), d)
  return w


def apsp(w):
  """The shortest-path lengths [n, n] of the graph whose edge lengths are `w` (>= 0, +inf = no edge, the diagonal
  taken as 0), +inf where there is no path: Floyd-Warshall over k.  ValueError for a negative or NaN edge length."""
  be = context.get().backend
  fn = getattr(be, 'apsp', None)
  if fn is not None:
    return fn(w)
  return apsp_numpy(np.asarray(be.to_numpy(w)))


def apsp_numpy(w):
  """apsp on a host array (which is not written)."""
  d = np.array(w)
  _, n = tile_checks.check_apsp(d.dtype, d.shape)
  off = ~np.eye(n, dtype=bool)
  if np.any(~(d[off] >= 0)):
    raise ValueError('apsp: negative or NaN edge length')
  np.fill_diagonal(d, 0)
  for k in range(n):
    np.minimum(d, d[:, k, None] + d[None, k, :], out=d)      # (t replaces d only where t < d; inf + x never wins)
  return d
