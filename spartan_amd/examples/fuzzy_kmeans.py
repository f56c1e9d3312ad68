"""Fuzzy k-means (interface of the reference's spartan/examples/fuzzy_kmeans.py: `fuzzy_kmeans(points, k, num_iter, m,
centers)` -> labels, an expression).

Per iteration, with the whole centres C [k, d] on every row tile X [n, d] (fuzzy_kmeans.py:41-62, 83-93):

    dist_ij = |x_i - c_j|_2, 1e-10 where it is 0        p_ij = dist_ij ** (1 / (m - 1))
    u_ij = p_ij / sum_j p_ij                            labels_i = argmax_j u_ij  (first occurrence)
    w_ij = u_ij ** m        centers_j = sum_i w_ij x_i / sum_i w_ij

Behaviour of the reference that is kept because its recorded outputs (tests/golden/fuzzy_w4.npz) are the yardstick:
the membership GROWS with the distance (the reference raises the distance, not its inverse, to 1 / (m - 1)), so a
point's label is its FARTHEST centre and the centres are pulled towards the points far from them.  This is the
reference, not textbook fuzzy c-means.

Two ways of phrasing an iteration:

  'fused'   (default) one shuffle whose mapper calls _fuzzy.fuzzy_step on its tile (HipBackend: sp_fuzzy_step --
            distances, memberships and the weighted sums in one fused pass) and updates three targets: sums (k, d) and
            wsum (k, 1), single-tile arrays with reduce_fn=np.add, and labels; then centers = sums / wsum on the driver.
            Nothing of size n x k is allocated: at 1.25 M points and k = 1024 that matrix is 5 GB per tile in float32.
  'map2'    the reference's structure: fuzzy = map2(points) as a distributed [n, k] array (its tile body is the
            kernel's U output), labels = argmax(fuzzy, axis=1), the centres from a second map2 over (points, fuzzy)
            with reducer=np.add on the tiles' `**` and `dot`, divided by sum(fuzzy ** m, axis=0).

Deviations from the reference: `points` may be float32 (the run is then in float32; integer points are converted to
float64 on the device); m <= 1 (the reference divides by zero or inverts the exponent's sign silently), k < 1 and
num_iter < 1 raise ValueError; `implementation` and `full_output` are additions."""
import numpy as np

from .. import context, expr
from ..array import distarray, extent
from . import _fuzzy

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _tile_in(points, dtype):
  return points if isinstance(points, distarray.Absent) else context.get().backend.astype(points, dtype)


def _fused_mapper(inputs, ex, d_pts, centers, m, dtype, sums, wsum, labels):
  """Tile body of 'fused': all three products of one tile, pushed into their targets."""
  points = _tile_in(d_pts.fetch(ex), dtype)
  k = centers.shape[0]
  tile_labels, tile_sums, tile_wsum = _fuzzy.fuzzy_step(points, centers, m)
  sums.update(extent.from_shape(sums.shape), tile_sums)
  wsum.update(extent.from_shape(wsum.shape), tile_wsum.reshape(k, 1))
  labels.update(extent.create((ex.ul[0],), (ex.lr[0],), labels.shape), tile_labels)
  return []


def _membership_mapper(extents, tiles, centers=None, m=None, dtype=None):
  """Tile body of 'map2', first join: the memberships of this row band against all centres."""
  ex = extents[0]
  k = centers.shape[0]
  target = extent.create((ex.ul[0], 0), (ex.lr[0], k), (ex.array_shape[0], k))
  yield target, _fuzzy.fuzzy_step(_tile_in(tiles[0], dtype), centers, m, want_u=True)[3]


def _center_mapper(extents, tiles, shape=None, m=None, dtype=None):
  """Tile body of 'map2', second join: the reference's dot(X.T, fuzzy ** m).T of this row band, formed as
  dot((fuzzy ** m).T, X) so that the partial is a dense [k, d] tile and not a transposed view of a [d, k] one."""
  points, fuzzy = _tile_in(tiles[0], dtype), tiles[1]
  weights = fuzzy ** np.dtype(dtype).type(m)
  yield extent.create((0, 0), shape, shape), weights.T.dot(points)


_membership_mapper.yields_fresh_tensors = True      # the kernel's output (or NumPy's), never a fetched tile
_center_mapper.yields_fresh_tensors = True


def fuzzy_kmeans(points, k=10, num_iter=10, m=2.0, centers=None, implementation='fused', full_output=False):
  """Labels (an expression of shape (n,), int64) after `num_iter` iterations on `points` (expression / distributed
  array / NumPy array, tiled by rows) with `k` centres and fuzzifier `m` > 1.  centers: the start, a NumPy array or an
  expression of shape (k, d) (default: the reference's expr.rand(k, d)).  full_output: (labels, centers), the centres
  a NumPy array.  See the module docstring for the two implementations and the reference's meaning of a label."""
  m = _fuzzy.check_m(m, 'fuzzy_kmeans')
  k, num_iter = int(k), int(num_iter)
  if k < 1:
    raise ValueError('fuzzy_kmeans: k = %d must be at least 1' % k)
  if num_iter < 1:
    raise ValueError('fuzzy_kmeans: num_iter = %d' % num_iter)
  if implementation not in ('fused', 'map2'):
    raise ValueError('fuzzy_kmeans: unknown implementation %r' % (implementation,))
  if isinstance(points, np.ndarray):
    points = expr.from_numpy(points)
  if len(points.shape) != 2:
    raise ValueError('fuzzy_kmeans: expected points of shape (n, d), got %s' % (tuple(points.shape),))
  n, dim = (int(v) for v in points.shape)
  points = points.evaluate() if hasattr(points, 'evaluate') else points
  dtype = np.dtype(points.dtype) if np.dtype(points.dtype) in _FLOATS else np.dtype(np.float64)
  if centers is None:
    centers = expr.rand(k, dim)
  if tuple(centers.shape) != (k, dim):
    raise ValueError('fuzzy_kmeans: centers of shape %s for k = %d and %d features' % (tuple(centers.shape), k, dim))

  labels = expr.zeros((n,), dtype=np.int64) if implementation == 'fused' else None
  for _ in range(num_iter):
    if not isinstance(centers, np.ndarray):
      centers = centers.glom()
    centers = np.ascontiguousarray(centers, dtype=dtype)
    if implementation == 'fused':
      sums = expr.ndarray((k, dim), dtype=dtype, reduce_fn=np.add, tile_hint=(k, dim))
      wsum = expr.ndarray((k, 1), dtype=dtype, reduce_fn=np.add, tile_hint=(k, 1))
      expr.shuffle(points, _fused_mapper,
                   kw={'d_pts': points, 'centers': centers, 'm': m, 'dtype': dtype, 'sums': sums, 'wsum': wsum,
                       'labels': labels},
                   shape_hint=(1,)).evaluate()
      with np.errstate(all='ignore'):
        centers = sums.glom() / wsum.glom()
    else:
      fuzzy = expr.map2(points, 0, fn=_membership_mapper, fn_kw={'centers': centers, 'm': m, 'dtype': dtype},
                        shape=(n, k), dtype=dtype)
      labels = expr.argmax(fuzzy, axis=1)
      new_centers = expr.map2((points, fuzzy), (0, 0), fn=_center_mapper,
                              fn_kw={'shape': (k, dim), 'm': m, 'dtype': dtype}, shape=(k, dim), dtype=dtype,
                              reducer=np.add, tile_hint=(k, dim))
      centers = new_centers / expr.reshape(expr.sum(fuzzy ** dtype.type(m), axis=0), (k, 1))
  if not full_output:
    return labels
  if not isinstance(centers, np.ndarray):
    centers = centers.glom()
  return labels, np.asarray(centers)
