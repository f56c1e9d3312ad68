"""Canopy clustering (interface of the reference's spartan/examples/canopy_clustering.py: `canopy_cluster(points, t1,
t2, cf)` -> the lazy labels (n,) int32, and `find_centers`; its tests/test_canopy_clustering.py is the benchmark).

With points (n, d) (canopy_clustering.py:129-143):

    every row tile walks its rows in order (:33-65, _canopy_mapper): a canopy whose CREATING row is within t1 (squared
        distance, strict <) observes the row (count += 1, sum += row); a row within t2 of no creating row becomes a
        canopy.  The tile gives the means sum / count of its canopies with count > cf.
    find_centers (:95-126) runs the same loop on the host over all tiles' means, one after the other.
    every row gets the lowest j at which 1 / (1 + |x - c_j|^2) is largest (:68-92, _cluster_mapper).

The reference runs both tile bodies one interpreted row and one interpreted canopy at a time.  Here the first is ONE
tile_operation whose body is _canopy.canopy (HipBackend: sp_canopy, a chain's whole loop in one workgroup, exactly the
sequential loop's result), find_centers is the same body with one chain on the concatenated means, and the labels are a
lazy shuffle whose body is one _canopy.pdf_label (sp_pdf_label) into an (n,) int32 target.
include/spartan_hip_canopy.h states the arithmetic; everything is the reference's, operation for operation.

find_centers takes the tiles' results in ascending order of each tile's first row.  The reference takes them in the
order of a dict's values(), which is arbitrary; for one tile, and whenever that order happens to be ascending, the two
agree.  A tile that does not hold whole rows makes the driver retile to row bands of divup(n, workers) first.

Additions: float32 points run in float32 (points of any other real dtype are converted to float64);
`chains_per_tile` = c cuts every tile into c consecutive chains, each with its own list of canopies -- mathematically
the reference run on c times as many tiles; `return_centers` gives (labels, centers).  No tile result at all gives
centers of shape (0, d) and labels of -1.  Deviations: points that are not 2-D, d < 1, chains_per_tile < 1, thresholds
that are not finite and a cf that is not an integer raise ValueError; complex or object arrays raise TypeError."""
import numpy as np

from .. import context, expr, tile_checks, util
from ..array import distarray, extent
from . import _canopy

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _canopy_mapper(array, ex, t1=None, t2=None, cf=None, chains=None):
  """Tile body of the first pass: (the tile's first row, the means of its canopies with count > cf)."""
  if ex.ul[1] != 0:                     # (never after the driver's retile)
    return []
  centers, counts, _ = _canopy.canopy(array.fetch(ex), t1, t2, chains=chains)
  if isinstance(centers, distarray.Absent):
    return [(None, (ex.ul[0], None))]
  return [(None, (ex.ul[0], centers[counts > cf]))]


def _cluster_mapper(array, ex, centers=None):
  """Tile body of the labels: the band's rows of the (n,) target."""
  if ex.ul[1] != 0:
    return []
  n = array.shape[0]
  return [(extent.create((ex.ul[0],), (ex.lr[0],), (n,)), _canopy.pdf_label(array.fetch(ex), centers))]


_cluster_mapper.yields_fresh_tensors = True      # the kernel's output (or NumPy's), never a fetched tile


def find_centers(blocks, t1, t2, cf):
  """The final centres [k, d] from `blocks`, the tiles' centres as a list of [m_i, d] host arrays of one float dtype:
  the canopy loop with one chain over their concatenation, in the order given, then the means of the canopies with
  count > cf.  (The reference takes the blocks in a dict's values() order, which is arbitrary; canopy_cluster gives
  them in ascending order of each tile's first row.)  No block gives an array of shape (0, 0)."""
  blocks = [np.asarray(b) for b in blocks]
  if not blocks:
    return np.zeros((0, 0))
  points = np.ascontiguousarray(np.concatenate(blocks, axis=0))
  _, _, _, t1, t2, _, _, cf = tile_checks.check_canopy(points.dtype, points.shape, t1, t2, cf=cf, what='find_centers')
  centers, counts, _ = _canopy.canopy(points, t1, t2, chains=1)
  return np.ascontiguousarray(np.asarray(centers)[np.asarray(counts) > cf])


def canopy_cluster(points, t1=0.1, t2=0.1, cf=1, chains_per_tile=1, return_centers=False):
  """The cluster label of every row of `points` (expression / distributed array / NumPy array of shape (n, d)) as a
  lazy expression of shape (n,), int32 -- or (labels, centers [k, d] host array) with `return_centers`: canopies with
  the thresholds t1 (observe) and t2 (bind) on the SQUARED distance, of more than `cf` rows.  See the module docstring
  for the loop, `chains_per_tile` and the errors."""
  if isinstance(points, np.ndarray):
    if np.dtype(points.dtype).kind not in 'fiub':
      raise TypeError('canopy_cluster: points of dtype %s; the array holds real numbers' % np.dtype(points.dtype))
    points = expr.from_numpy(points)
  if len(points.shape) != 2:
    raise ValueError('canopy_cluster: expected points of shape (n, d), got %s' % (tuple(points.shape),))
  points = expr.evaluate(points)
  if np.dtype(points.dtype).kind not in 'fiub':
    raise TypeError('canopy_cluster: points of dtype %s; the array holds real numbers' % np.dtype(points.dtype))
  if np.dtype(points.dtype) not in _FLOATS:
    points = expr.evaluate(expr.astype(points, np.float64))
  dt, n, d, t1, t2, chains, _, cf = tile_checks.check_canopy(points.dtype, points.shape, t1, t2, chains_per_tile, cf=cf,
                                                             what='canopy_cluster')
  band = max(util.divup(n, context.get().num_workers), 1)
  if any(ex.ul[1] != 0 or ex.lr[1] != d for ex in points.tiles):
    points = expr.evaluate(expr.retile(points, tile_hint=(band, d)))

  found = expr.tile_operation(points, _canopy_mapper, kw={'t1': t1, 't2': t2, 'cf': cf, 'chains': chains}).evaluate()
  blocks = sorted((v for values in found.values() for v in (values or ()) if v[1] is not None), key=lambda v: v[0])
  centers = find_centers([np.zeros((0, d), dt)] + [b for _, b in blocks], t1, t2, cf)
  target = expr.ndarray((n,), dtype=np.int32, tile_hint=(band,))
  labels = expr.shuffle(points, _cluster_mapper, target=target, kw={'centers': centers})
  return (labels, centers) if return_centers else labels
