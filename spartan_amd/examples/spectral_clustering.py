"""Spectral clustering (interface of the reference's spartan/examples/spectral_clustering.py:
`spectral_cluster(points, k, num_iter, similarity_measurement)` -> labels, an expression).

The reference's pipeline (spectral_clustering.py:61-140), kept step by step:

    A_ij = measure(p_i, p_j)                  D_i = sum_j A_ij            s_i = 1 / sqrt(D_i), 1 where D_i is 0
    L = diag(s) A diag(s), then EVERY DIAGONAL ENTRY OF L SET TO 1
    d, S = lanczos.solve(L, L, min(2 k, n), True)       U = S[:, :k]     init = U[argmax(U, axis=0)]
    labels = KMeans(k, num_iter).fit(U, init)

Behaviour of the reference that is kept because its recorded outputs (tests/golden/spectral_w4.npz) are the yardstick:
the diagonal of L is overwritten with 1 AFTER the normalisation, so with 'rbf' the leading eigenvalues are about 1.93
and not 1; `spectral_cluster` never passes a gamma, so the reference's 'rbf' is exp(-d2).

Where the reference fills A by a Python double loop over all pairs, sums its rows and scales it in a second pass, the
affinity matrix is never stored here.  The points (n x d, small beside n x n) are glommed once; every row band of
them runs _spectral.affinity_degree against the whole set (HipBackend: sp_affinity_degree, the affinities stay in
registers) in a shuffle into a (n,) target; the host forms s in the run's dtype as the reference does (sqrt, zeros to
1, 1.0 / ...); a second shuffle writes L's row bands with _spectral.affinity_matrix(..., scale=s) (sp_affinity_matrix:
the affinities recomputed, L written exactly once).  L_ij = a_ij * (s_i * s_j), which differs from the reference's
(s_i a_ij) s_j by a rounding and makes L symmetric bit for bit; its bits do not depend on the number of workers.

Measures: 'rbf' exp(-gamma d2), 'euclidean' sqrt(d2), 'manhattan' sum_f |x_f - y_f|.

Deviations from the reference: `points` may be float32 (the run is then in float32; integer points are converted to
float64); `gamma`, `dtype` and `full_output` are additions; 'scaled_euclidean' raises NotImplementedError (the
reference calls np.square(X, Y), which writes X squared into its second operand: its result depends on the order in
which the pairs are visited, which is not a behaviour one can keep); k < 1, num_iter < 1, k > n and points that are
not 2-D raise ValueError; the k-means fit is given reducer=np.add (the real update of the centres: with the
reference's default the last tile's partial sums replace the others', and the outcome with several workers then
depends on the arbitrary sign numpy.linalg.eig gives the Ritz vectors, which decides the starting rows)."""
import numpy as np

from .. import context, expr, tile_checks
from ..array import distarray, extent
from . import _spectral, lanczos
from .sklearn.cluster.k_means_ import KMeans

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _band(array, ex, dtype):
  """The whole rows of the tile `ex` of the points, in the run's dtype; None for a tile that does not start a row band
  (points that are cut by columns as well)."""
  if ex.ul[1] != 0:
    return None
  rows = extent.create((ex.ul[0], 0), (ex.lr[0], array.shape[1]), array.shape)
  band = array.fetch(rows)
  return band if isinstance(band, distarray.Absent) else context.get().backend.astype(band, dtype)


def _degree_mapper(array, ex, all_points=None, metric=None, gamma=None, dtype=None):
  """Tile body of the first shuffle: the degrees of this row band against all points."""
  band = _band(array, ex, dtype)
  if band is not None:
    n = array.shape[0]
    yield extent.create((ex.ul[0],), (ex.lr[0],), (n,)), _spectral.affinity_degree(band, all_points, metric, gamma)


def _matrix_mapper(array, ex, all_points=None, metric=None, gamma=None, dtype=None, scale=None):
  """Tile body of the second shuffle: this row band of L (with `scale`) or of the plain A (without)."""
  band = _band(array, ex, dtype)
  if band is not None:
    n = array.shape[0]
    yield (extent.create((ex.ul[0], 0), (ex.lr[0], n), (n, n)),
           _spectral.affinity_matrix(band, ex.ul[0], all_points, metric, gamma, scale=scale))


_degree_mapper.yields_fresh_tensors = True      # the kernel's output (or NumPy's), never a fetched tile
_matrix_mapper.yields_fresh_tensors = True


def _prepare(points, metric, gamma, dtype, what):
  """(points as an evaluated array, the same on the host in the run's dtype, gamma, dtype)."""
  gamma = _spectral.check_params(metric, gamma, what)
  if isinstance(points, np.ndarray):
    points = expr.from_numpy(points)
  if len(points.shape) != 2:
    raise ValueError('%s: expected points of shape (n, d), got %s' % (what, tuple(points.shape),))
  points = points.evaluate() if hasattr(points, 'evaluate') else points
  if dtype is None:
    own = np.dtype(points.dtype)
    dtype = own if own in _FLOATS else np.dtype(np.float64)
  dtype = tile_checks.check_float_dtype(dtype, what)
  host = np.ascontiguousarray(np.asarray(points.glom()), dtype=dtype)
  return points, host, gamma, dtype


def affinity_matrix(points, metric='rbf', gamma=1.0, dtype=None):
  """The plain affinity matrix A [n, n] of `points` [n, d] as a row-tiled expression (the kernel without a scale)."""
  points, host, gamma, dtype = _prepare(points, metric, gamma, dtype, 'affinity_matrix')
  n = int(points.shape[0])
  return expr.shuffle(points, _matrix_mapper,
                      kw={'all_points': host, 'metric': metric, 'gamma': gamma, 'dtype': dtype}, shape_hint=(n, n))


def _laplacian(points, host, metric, gamma, dtype):
  """(L [n, n] evaluated, tiled by the row bands of `points`; the degrees D [n] on the host)."""
  n = int(points.shape[0])
  kw = {'all_points': host, 'metric': metric, 'gamma': gamma, 'dtype': dtype}

  # the degrees: nothing of size n x n is stored
  degrees = expr.shuffle(points, _degree_mapper, kw=kw, target=expr.ndarray((n,), dtype=dtype, tile_hint=(n,)))
  D = np.asarray(degrees.glom())

  # the scales, on the host in the run's dtype as the reference forms them
  scale = np.sqrt(D)
  scale[scale == 0] = 1
  scale = (1.0 / scale).astype(dtype)

  # the normalised matrix, written once
  L = expr.shuffle(points, _matrix_mapper, kw=dict(kw, scale=scale), shape_hint=(n, n)).evaluate()
  return L, D


def laplacian(points, metric='rbf', gamma=1.0, dtype=None):
  """(L, D): the normalised affinity matrix diag(s) A diag(s) with a diagonal of 1, an evaluated row-tiled array, and
  the degrees D [n], a NumPy array -- what spectral_cluster hands to the Lanczos iteration."""
  points, host, gamma, dtype = _prepare(points, metric, gamma, dtype, 'laplacian')
  return _laplacian(points, host, metric, gamma, dtype)


def spectral_cluster(points, k=10, num_iter=10, similarity_measurement='rbf', gamma=1.0, dtype=None,
                     full_output=False):
  """Labels (an expression) of `points` (expression / distributed array / NumPy array of shape (n, d), tiled by rows)
  in `k` clusters: k-means with `num_iter` iterations on the k leading Ritz vectors of the normalised affinity matrix.
  full_output: (labels, d, U, D) with the min(2 k, n) Ritz values d, the (n, k) matrix U that was clustered and the
  degrees D, NumPy arrays.  See the module docstring for the reference's behaviour that is kept and for the
  additions."""
  k, num_iter = int(k), int(num_iter)
  if k < 1:
    raise ValueError('spectral_cluster: k = %d must be at least 1' % k)
  if num_iter < 1:
    raise ValueError('spectral_cluster: num_iter = %d' % num_iter)
  metric = similarity_measurement
  points, host, gamma, dtype = _prepare(points, metric, gamma, dtype, 'spectral_cluster')
  n = int(points.shape[0])
  if k > n:
    raise ValueError('spectral_cluster: k = %d clusters for %d points' % (k, n))
  L, D = _laplacian(points, host, metric, gamma, dtype)

  overshoot = min(k * 2, n)
  d, U = lanczos.solve(L, L, overshoot, True)
  U = np.ascontiguousarray(U[:, 0:k])

  # the rows that hold the largest entry of each column start the clusters
  init_clusters = U[np.argmax(U, axis=0)]
  # (reducer=np.add: the tiles' partial counts and sums are added.  The reference's fit leaves the LAST tile's partial
  #  in place of the others, see k_means_.py; the sign LAPACK gives the Ritz vectors is arbitrary and flips under a
  #  change of 1e-16 in L, one of the two signs starts two clusters in the same group here, and with several workers
  #  only the real update recovers from that start.)
  _, labels = KMeans(k, num_iter).fit(expr.from_numpy(U), init_clusters, reducer=np.add)
  if not full_output:
    return labels
  return labels, d, U, D
