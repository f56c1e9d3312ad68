"""Isomap embedding (interface of the reference's spartan/examples/sklearn/manifold/isomap.py:
`Isomap(n_neighbors, n_components, ...).fit(X)` -> embedding_, dist_matrix_, training_data_, nbrs_).

  neighbours     the project's own NearestNeighbors with n_neighbors + 1 (the fitted points are their own queries); per
                 row the entry whose index is the row itself is dropped -- where duplicate points pushed the row out of
                 its own list, the last entry.  (The reference hands the same job to scikit-learn's kneighbors_graph.)
  graph          backend.graph_from_knn (sp_graph_from_knn): the dense undirected graph, +inf = no edge
  geodesics      backend.apsp (sp_apsp): blocked Floyd-Warshall in the (min, +) semiring on the device.  The reference
                 runs a Dijkstra per source row (sklearn/util/graph_shortest_path.pyx), each worker a band of rows.
                 dist_matrix_ is the result with +inf replaced by 0 -- the reference's convention: its matrix starts as
                 zeros and unreached targets stay 0.
  embedding      G = -0.5 dist_matrix_^2, double-centred (row means and column means subtracted, the grand mean added:
                 map and reduce kernels on the device tile); (w, V) = syev(G) (sp_syevj); the n_components largest
                 eigenvalues, descending, their vectors taken through one refinement step (_refine: a Jacobi solver
                 leaves them about n u from the truth where LAPACK leaves a few u);
                 embedding_ = V sqrt(w), a column of zeros where the eigenvalue is <= 0.  (The reference calls
                 scikit-learn's KernelPCA with a precomputed kernel: the same recipe.)

eigen_solver: 'auto' and 'dense' are the syev route.  'arpack' raises NotImplementedError: the project has no iterative
eigensolver, and 'dense' is the one to ask for.  tol and max_iter are accepted and unused, as they are for 'dense' in the
reference.  n_neighbors is at most 127 (n_neighbors + 1 must stay within the neighbour kernel's 128).

In a multi-rank job every rank runs the graph, the shortest paths and the eigenproblem on the whole matrix (the
neighbour driver already merges at driver level on every rank); a distance matrix spread over devices is out of
scope.  embedding_ is practical up to the orders the Jacobi eigensolver handles (a few thousand points); dist_matrix_
alone goes far beyond them -- fit(X, embed=False) stops after it.
"""
import numpy as np

from .... import context, tile_checks
from ... import _dense
from ..neighbors import NearestNeighbors
from . import _graph

MAX_NEIGHBORS = 127


class Isomap(object):
  """n_neighbors: neighbours per point in the graph; n_components: coordinates of the embedding; eigen_solver:
  'auto' | 'dense' ('arpack' is refused); neighbors_algorithm: passed to NearestNeighbors (module docstring)."""

  def __init__(self, n_neighbors=5, n_components=2, eigen_solver='auto', tol=0, max_iter=None,
               neighbors_algorithm='auto'):
    self.n_neighbors = n_neighbors
    self.n_components = n_components
    self.eigen_solver = eigen_solver
    self.tol = tol
    self.max_iter = max_iter
    self.neighbors_algorithm = neighbors_algorithm
    self.nbrs_ = NearestNeighbors(n_neighbors=n_neighbors, algorithm=neighbors_algorithm)

  def _neighbour_lists(self, X):
    """(dist, idx), host arrays [n, n_neighbors]: every point's neighbours without the point itself."""
    k = int(self.n_neighbors)
    self.nbrs_.fit(X)
    self.training_data_ = self.nbrs_.X
    dist, ind = self.nbrs_.kneighbors(self.nbrs_.X, n_neighbors=k + 1)
    self.nbrs_.n_neighbors = k          # (kneighbors keeps the k of its last call)
    n = dist.shape[0]
    own = ind == np.arange(n, dtype=np.int64)[:, None]
    drop = np.where(own.any(axis=1), own.argmax(axis=1), k)
    keep = np.ones(ind.shape, bool)
    keep[np.arange(n), drop] = False
    return np.ascontiguousarray(dist[keep].reshape(n, k)), np.ascontiguousarray(ind[keep].reshape(n, k))

  def fit(self, X, embed=True):
    """X: expression / array / NumPy array of shape (n_samples, n_features).  Sets nbrs_, training_data_, dist_matrix_
    (host, (n, n)) and -- unless embed is false -- embedding_ (host, (n, n_components)).  Returns self."""
    if self.eigen_solver == 'arpack':
      raise NotImplementedError("eigen_solver='arpack': there is no iterative eigensolver here; use 'dense'")
    if self.eigen_solver not in ('auto', 'dense'):
      raise ValueError('unknown eigen_solver %r' % (self.eigen_solver,))
    k = tile_checks.check_count('n_neighbors', self.n_neighbors, MAX_NEIGHBORS)
    be = context.get().backend
    dist, ind = self._neighbour_lists(X)
    graph = _graph.graph_from_knn(dist, ind)
    geo = _graph.apsp(graph)
    geo = np.where(geo < np.inf, geo, geo.dtype.type(0))                # (a device tile's operators are the fused map kernel)
    self.dist_matrix_ = np.asarray(be.to_numpy(geo))
    if not embed:
      return self
    G = geo * geo * -0.5
    G = G - G.mean(axis=1, keepdims=True) - G.mean(axis=0, keepdims=True) + G.mean()
    w, vecs = _dense.syev(G)
    w = np.asarray(be.to_numpy(w))
    m = min(int(self.n_components), w.shape[0])
    cols = np.arange(w.shape[0] - 1, w.shape[0] - 1 - m, -1)          # the m largest eigenvalues, descending
    lam, chosen = _refine(G, vecs, w, cols, be)
    scale = np.sqrt(np.where(lam > 0, lam, 0)).astype(chosen.dtype)
    self.embedding_ = np.ascontiguousarray(chosen * scale)
    return self


def _refine(G, vecs, w, cols, be):
  """(eigenvalues, eigenvectors [n, m]) of the columns `cols` of the eigendecomposition (w, vecs) of G after one step
  of the refinement of Ogita and Aishima (2018), for the chosen columns only: with V = vecs, V_m = vecs[:, cols],

      R = I_m - V^T V_m,   S = V^T (G V_m),   l_j = S_jj / (1 - R_jj),
      E_ij = (S_ij + l_j R_ij) / (l_j - w_i)  (i != j),   E_jj = R_jj / 2,   V_m <- V_m + V E.

  A Jacobi solver stops once the off-diagonal norm is below n u |G|_F and its V is a product of O(n^2) rotations per
  sweep: both leave a chosen eigenvector about n u (times |G|_F / gap) from the true one, where LAPACK leaves a few u.
  The step costs four products with an n x m matrix (the GEMM kernel on device tiles) and is quadratically
  convergent: what remains is the rounding of these products.  Terms whose denominator is within n u |G|_F are left out:
  within a cluster of equal eigenvalues any basis is as good."""
  vecs_host = np.asarray(be.to_numpy(vecs))
  chosen = np.ascontiguousarray(vecs_host[:, cols])
  n, m = w.shape[0], cols.size
  if n < 2 or m == 0:
    return w[cols], chosen
  vt = np.transpose(vecs)
  own = (cols, np.arange(m))
  R = -np.asarray(be.to_numpy(vt.dot(chosen))).astype(np.float64)           # [n, m]: R[i][j] = delta - v_i . v_cols[j]
  R[own] += 1.0
  S = np.asarray(be.to_numpy(vt.dot(G.dot(chosen)))).astype(np.float64)     # [n, m]: S[i][j] = v_i . G v_cols[j]
  lam = S[own] / (1.0 - R[own])
  w64 = w.astype(np.float64)
  denom = lam[None, :] - w64[:, None]
  tiny = np.abs(denom) <= n * (np.finfo(w.dtype).eps / 2) * np.sqrt(np.sum(w64 ** 2))
  E = np.where(tiny, 0.0, (S + lam[None, :] * R) / np.where(tiny, 1.0, denom))
  E[own] = R[own] / 2
  chosen = chosen + np.asarray(be.to_numpy(vecs.dot(np.ascontiguousarray(E.astype(w.dtype)))))
  return lam.astype(w.dtype), np.ascontiguousarray(chosen.astype(w.dtype))
