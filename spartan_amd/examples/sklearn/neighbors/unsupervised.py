"""Unsupervised nearest-neighbour search (interface of the reference's spartan/examples/sklearn/neighbors/
unsupervised.py: `NearestNeighbors(n_neighbors, algorithm).fit(X).kneighbors(Q, n_neighbors)` -> (dist, ind)).

  'auto', 'kd_tree', 'ball_tree'   the reference's per-tile scheme (its _knn_mapper and the selection on the master):
                 every row band of X yields k candidates per query with global row numbers, and the candidates of all
                 bands are merged.  The reference searches a band with scikit-learn's trees; here the band goes through
                 backend.knn (sp_knn: distance and top-k in one pass) and the merge through backend.knn_merge
                 (sp_knn_merge).  All of them are exact searches: the answers are the same.  Q is fetched whole by
                 every band; of a column-cut X only the tile at column 0 works, on its whole row band; everything
                 stays on the device until the final (nq, k) result, whose square root is the map kernel's.
  'brute'        the reference's pure-expression phrasing: reshape, subtract, square, sum(axis=2), argsort, sort, first k
                 columns, sqrt.  It writes all nq x np distances and sorts every row twice: kept, as k-means keeps its
                 'broadcast' variant, because it exercises the map / reduce / sort path and is the yardstick for the
                 fused one.  (Its indices pass through the dtype of X, as the reference's argsort target does: exact
                 below 2^24 rows in float32.)

Distances are Euclidean; neighbours at equal distance come in ascending row order.  Deviations from the reference:
'auto' takes the per-tile scheme (the reference's takes 'brute'), and the column cut of 'brute' uses self.n_neighbors
(the reference uses the raw argument, None by default).
"""
import numpy as np

from .... import context, expr
from ....array import distarray, extent
from ....context import LocalKernelResult
from . import _knn


def _knn_mapper(ex, X=None, Q=None, k=None, slots=None, cand_dist2=None, cand_idx=None):
  """Tile body: the k candidates of every query in the row band of X that starts with this tile, into the band's k
  columns of the two candidate arrays."""
  if ex.ul[1] != 0:                   # a column-cut X: the tile at column 0 does the work of its row band
    return LocalKernelResult(result=[])
  band = extent.create((ex.ul[0], 0), (ex.lr[0], X.shape[1]), X.shape)
  points = X.fetch(band)
  queries = Q.fetch(extent.from_shape(Q.shape))
  dist2, idx = _knn.knn(queries, points, k, index_offset=ex.ul[0])
  slot = slots[ex.ul[0]]
  where = extent.create((0, slot * k), (Q.shape[0], (slot + 1) * k), cand_dist2.shape)
  cand_dist2.update(where, dist2, wait=False, owned=True)
  cand_idx.update(where, idx, wait=False, owned=True)
  return LocalKernelResult(result=[])


class NearestNeighbors(object):
  """n_neighbors: the default k of kneighbors; algorithm: 'auto' | 'kd_tree' | 'ball_tree' | 'brute' (module docstring)."""

  def __init__(self, n_neighbors=5, algorithm='auto'):
    self.n_neighbors = n_neighbors
    self.algorithm = algorithm

  def fit(self, X):
    """X: expression / array / NumPy array of shape (n_samples, n_features)."""
    if isinstance(X, np.ndarray):
      X = expr.from_numpy(X)
    self.X = X
    return self

  def kneighbors(self, X, n_neighbors=None):
    """(dist, ind), host arrays of shape (n_queries, k): the Euclidean distances to the k nearest fitted points of
    every row of X, ascending, and the rows of those points (int64).  n_neighbors replaces the constructor's k, for
    this and later calls (as in the reference).  ValueError if k exceeds the number of fitted points."""
    if n_neighbors is not None:
      self.n_neighbors = n_neighbors
    Q = expr.from_numpy(X) if isinstance(X, np.ndarray) else X
    k = int(self.n_neighbors)
    if len(Q.shape) != 2 or len(self.X.shape) != 2 or Q.shape[1] != self.X.shape[1]:
      raise ValueError('kneighbors: queries of shape %s against points of shape %s' % (tuple(Q.shape), tuple(self.X.shape)))
    if k < 1:
      raise ValueError('Expected n_neighbors > 0. Got %d' % k)
    if k > self.X.shape[0]:
      raise ValueError('Expected n_neighbors <= n_samples,  but n_samples = %d, n_neighbors = %d' % (self.X.shape[0], k))
    if self.algorithm == 'brute':
      return self._brute(Q, k)
    if self.algorithm in ('auto', 'kd_tree', 'ball_tree'):
      return self._tiles(Q, k)
    raise ValueError('unknown algorithm %r' % (self.algorithm,))

  def _brute(self, Q, k):
    X = self.X
    q3 = expr.reshape(Q, (Q.shape[0], 1, Q.shape[1]))
    x3 = expr.reshape(X, (1, X.shape[0], X.shape[1]))
    distances = expr.sum(expr.square(q3 - x3), axis=2)
    from .... import argsort, sort          # (the sort family resolves on first use, not with the package)
    ind = argsort(distances, axis=1)[:, :k].optimized().glom()
    dist = expr.sqrt(sort(distances, axis=1)[:, :k]).optimized().glom()
    return np.asarray(dist), np.asarray(ind).astype(np.int64)

  def _tiles(self, Q, k):
    be = context.get().backend
    nq = int(Q.shape[0])
    Xa, Qa = expr.evaluate(self.X), expr.evaluate(Q)
    dtype = np.dtype(Xa.dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
      dtype = np.dtype(np.float64)
    if nq == 0:
      return np.empty((0, k), dtype), np.empty((0, k), np.int64)
    if np.dtype(Xa.dtype) != dtype:
      Xa = expr.evaluate(expr.astype(Xa, dtype))
    if np.dtype(Qa.dtype) != dtype:
      Qa = expr.evaluate(expr.astype(Qa, dtype))
    slots = {lo: i for i, lo in enumerate(sorted(set(ex.ul[0] for ex in Xa.tiles if ex.ul[1] == 0)))}
    # one (nq, k) tile per row band in each candidate array: a band's update fills exactly one tile
    width = len(slots) * k
    cand_dist2 = distarray.create((nq, width), dtype, tile_hint=(nq, k))
    cand_idx = distarray.create((nq, width), np.int64, tile_hint=(nq, k))
    Xa.foreach_tile(mapper_fn=_knn_mapper, kw=dict(X=Xa, Q=Qa, k=k, slots=slots, cand_dist2=cand_dist2,
                                                   cand_idx=cand_idx))
    # driver level: every rank fetches every band's candidates and merges them
    whole = extent.from_shape((nq, width))
    dist2, idx = cand_dist2.fetch(whole), cand_idx.fetch(whole)
    if len(slots) > 1:
      dist2, idx = _knn.knn_merge(dist2, idx, k)
    dist = np.sqrt(dist2)                # (a device tile's ufunc is the fused map kernel)
    return np.asarray(be.to_numpy(dist)), np.asarray(be.to_numpy(idx)).astype(np.int64, copy=False)
