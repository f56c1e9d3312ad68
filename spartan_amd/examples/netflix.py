"""Stochastic-gradient matrix factorisation of a rating matrix, the "Netflix" example (interface of the reference's
spartan/examples/netflix.py: `sgd(V, M, U)` -> an object whose `evaluate()` / `force()` runs one epoch and updates `M`
and `U` in place; `fake_netflix_mapper` fills a sparse array with Netflix-like data; its tests/test_netflix.py and
tests/benchmark_netflix.py read the same here).  The algorithm is the stratified SGD of the Sparkler paper.

    V (users, movies) sparse, cut into a grid of blocks;  U (users, r);  M (movies, r);  V ~= U M^T

An epoch visits every block once.  The blocks are grouped into strata whose blocks share no block row and no block
column, so the blocks of a stratum touch disjoint rows of U and of M; the strata run one after the other, one shuffle
over V each.  A block's pass (netflix_core.pyx, _sgd_inner) walks its ratings (i, j, r) in order:

    d = r - U_i . M_j        U_i += (U_i d) lr        M_j += (M_j d) lr        lr = float32(1e-5)

(each factor row is scaled by itself: what the reference's compiled loop does).  The reference runs this loop one
rating at a time; here _netflix.sgd_mf runs it on the block's tile (HipBackend: sp_sgd_mf, level-scheduled -- ratings
that share neither row nor column run at once -- with the bits of the sequential loop; include/spartan_hip_mf.h states
the order of the inner product).  As in the reference the mapper takes its rows of U and M with `select` and writes
them back with `update_slice`.

The order of a block's ratings is the tile's stored order: rows ascending, columns ascending inside a row.  What an
upload makes of a mapper's COO block (sparse.from_scipy -> sp_coo_to_csr; on a NumPy backend scipy's sum_duplicates):
ratings at EQUAL coordinates are added into one rating -- the reference's loop would take them one after the other --
and an explicit zero stays a stored entry, a rating of 0 like any other.  fake_netflix_mapper yields both.

Strata.  The reference shuffles the tiles with Python's `random` and picks greedily, so no two interpreters agree.
Here the default is deterministic: for a grid of gr x gc blocks and g = max(gr, gc), stratum s = 0 .. g - 1 holds the
blocks (i, j) with (j - i) mod g == s, in row order.

Additions: `strata=` (a list of lists of block coordinates (i, j), validated: every block exactly once, no two blocks
of a stratum in one block row or block column); `lr=`; `want_error=` (after evaluate(), `.error` is the sum of |d| over
the epoch, each block's terms summed by the reduce kernel; the reference sums them into a float it discards);
`dtype=` (float32 or float64; default and only accepted value: the factors' dtype -- they are updated in place and
cannot be converted -- and V's values are converted to it once).  Deviations: a V that is not a sparse 2-D array
raises TypeError / ValueError, factors whose shapes do not fit V, a rank outside 1 .. 512 and factors whose tiling
cuts the rank dimension ValueError, factors that are not float32 / float64 or of two dtypes TypeError ("astype
first"), each naming the argument."""
import numpy as np

from .. import _hip, context, expr, tile_checks
from ..array import extent
from . import _netflix

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def fake_netflix_mapper(inputs, ex, p_rating=None):
  """Create "Netflix-like" data for the given extent (the reference's mapper, draw for draw).

  :param p_rating: Sparsity factor (probability a given cell will have a rating)"""
  import scipy.sparse
  n_ratings = int(max(1, ex.size * p_rating))
  uids = np.random.randint(0, ex.shape[0], n_ratings)
  mids = np.random.randint(0, ex.shape[1], n_ratings)
  ratings = np.random.randint(0, 5, n_ratings).astype(np.float32)
  data = scipy.sparse.coo_matrix((ratings, (uids, mids)), shape=ex.shape)
  yield ex, data


def sgd_netflix_mapper(inputs, ex, V=None, M=None, U=None, worklist=None, lr=None, errors=None, cell=None):
  """Tile body of a stratum: the pass over block `ex` of V if it is on the worklist; with `errors` the block's sum of
  |d| goes to cell `cell[ex]` of that array."""
  if ex not in worklist:
    return []
  v = V.fetch(ex)
  rows, cols = ex[0].to_slice(), ex[1].to_slice()
  u = U.select(rows)      # size: (ex.shape[0] * r)
  m = M.select(cols)      # size: (ex.shape[1] * r)
  err = _netflix.sgd_mf(v, u, m, lr=lr, want_error=errors is not None)
  U.update_slice(rows, u)
  M.update_slice(cols, m)
  if errors is None:
    return []
  at = cell[ex]
  return [(extent.create((at, 0), (at + 1, 1), errors.shape), err)]


def _cast_mapper(inputs, ex, dtype=None):
  yield ex, context.get().backend.sparse_blob(inputs.fetch(ex), dtype)


def _converted(V, dtype):
  """V with its values in `dtype`, tile for tile on the same grid (once per sgd object: the tiles keep their level
  schedules from then on)."""
  first = min(V.tiles, key=lambda ex: ex.ul)
  target = expr.sparse_empty(V.shape, dtype=dtype, tile_hint=first.shape)
  return expr.evaluate(expr.shuffle(V, _cast_mapper, target=target, kw={'dtype': np.dtype(dtype)}))


def default_strata(gr, gc):
  """Stratum s of a gr x gc grid: the blocks (i, j) with (j - i) mod max(gr, gc) == s, in row order."""
  g = max(gr, gc)
  return [[(i, j) for i in range(gr) for j in range(gc) if (j - i) % g == s] for s in range(g)]


def check_strata(strata, gr, gc):
  """`strata` as a list of lists of (i, j) tuples, or ValueError: a block outside the grid, a block that is missing or
  occurs twice, two blocks of one stratum in one block row or block column."""
  try:
    out = [[(int(i), int(j)) for i, j in stratum] for stratum in strata]
  except (TypeError, ValueError):
    raise ValueError('sgd: strata must be a list of lists of block coordinates (i, j)')
  seen = set()
  for s, stratum in enumerate(out):
    rows, cols = set(), set()
    for i, j in stratum:
      if not (0 <= i < gr and 0 <= j < gc):
        raise ValueError('sgd: strata[%d] names block (%d, %d) outside the %d x %d grid' % (s, i, j, gr, gc))
      if (i, j) in seen:
        raise ValueError('sgd: strata name block (%d, %d) twice' % (i, j))
      if i in rows or j in cols:
        raise ValueError('sgd: strata[%d] has two blocks that overlap in block row %d or block column %d' % (s, i, j))
      seen.add((i, j))
      rows.add(i)
      cols.add(j)
  if len(seen) != gr * gc:
    missing = sorted(set((i, j) for i in range(gr) for j in range(gc)) - seen)
    raise ValueError('sgd: strata miss %d of the %d blocks, the first (%d, %d)' % ((len(missing), gr * gc) + missing[0]))
  return out


class NetflixSGD(object):
  """One epoch over V, stratum by stratum; see the module docstring.  `strata` holds the block coordinates in use,
  `error` the epoch's sum of |d| after an evaluate() with want_error (None otherwise)."""

  def __init__(self, V, M, U, strata=None, lr=None, want_error=False, dtype=None):
    V = expr.evaluate(V) if isinstance(V, expr.Expr) else V
    if not getattr(V, 'sparse', False) or not hasattr(V, 'tiles'):
      raise TypeError('sgd: V must be a sparse distributed array (sparse_empty + shuffle), got %s' % type(V).__name__)
    if len(V.shape) != 2:
      raise ValueError('sgd: V must be 2-D (users, movies), got shape %s' % (tuple(V.shape),))
    M = expr.evaluate(M) if isinstance(M, expr.Expr) else M
    U = expr.evaluate(U) if isinstance(U, expr.Expr) else U
    for name, a in (('M', M), ('U', U)):
      if not hasattr(a, 'tiles') or getattr(a, 'sparse', False):
        raise TypeError('sgd: %s must be a dense distributed array, got %s' % (name, type(a).__name__))
      if np.dtype(a.dtype) not in _FLOATS:
        raise TypeError('sgd: %s of dtype %s is not supported (float32 float64); convert with astype first'
                        % (name, np.dtype(a.dtype)))
    if np.dtype(U.dtype) != np.dtype(M.dtype):
      raise TypeError('sgd: U and M of two dtypes (%s, %s); convert with astype first' % (np.dtype(U.dtype), np.dtype(M.dtype)))
    if len(U.shape) != 2 or U.shape[0] != V.shape[0]:
      raise ValueError('sgd: U of shape %s for a V of shape %s: expected (%d, r)' % (tuple(U.shape), tuple(V.shape), V.shape[0]))
    r = int(U.shape[1])
    if not 1 <= r <= _hip.SP_MF_MAX_F:
      raise ValueError('sgd: rank r = %d (of U) must be in 1 .. %d' % (r, _hip.SP_MF_MAX_F))
    if tuple(M.shape) != (V.shape[1], r):
      raise ValueError('sgd: M of shape %s for a V of shape %s and rank %d: expected (%d, %d)'
                       % (tuple(M.shape), tuple(V.shape), r, V.shape[1], r))
    for name, a in (('M', M), ('U', U)):
      if any(ex.ul[1] != 0 or ex.lr[1] != r for ex in a.tiles):
        raise ValueError('sgd: the tiling of %s cuts the rank dimension; tile it by rows (tile_hint=(rows, %d))' % (name, r))
    dt = np.dtype(U.dtype)
    if dtype is not None and tile_checks.check_float_dtype(dtype, 'sgd') != dt:
      raise TypeError('sgd: dtype = %s, but U and M are %s and are updated in place; convert with astype first'
                      % (np.dtype(dtype), dt))
    tile_checks.check_sgd_mf([dt] * 3, V.shape, U.shape, M.shape, lr, what='sgd')       # (lr)
    if np.dtype(V.dtype) != dt:
      V = _converted(V, dt)
    self.V, self.M, self.U, self.lr, self.want_error, self.dtype = V, M, U, lr, bool(want_error), dt
    self.row_starts = sorted(set(ex.ul[0] for ex in V.tiles))
    self.col_starts = sorted(set(ex.ul[1] for ex in V.tiles))
    gr, gc = len(self.row_starts), len(self.col_starts)
    self.blocks = {(self.row_starts.index(ex.ul[0]), self.col_starts.index(ex.ul[1])): ex for ex in V.tiles}
    if len(self.blocks) != gr * gc:
      raise ValueError('sgd: the tiles of V do not form a grid (%d tiles, %d x %d starts)' % (len(self.blocks), gr, gc))
    self.strata = default_strata(gr, gc) if strata is None else check_strata(strata, gr, gc)
    self.error = None

  def evaluate(self):
    errors = cell = None
    if self.want_error:
      n = len(self.blocks)
      errors = expr.evaluate(expr.zeros((n, 1), dtype=self.dtype, tile_hint=(n, 1)))
      cell = {ex: i * len(self.col_starts) + j for (i, j), ex in self.blocks.items()}
    for stratum in self.strata:
      worklist = set(self.blocks[b] for b in stratum)
      expr.shuffle(self.V, sgd_netflix_mapper, target=errors,
                   kw={'V': self.V, 'M': self.M, 'U': self.U, 'worklist': worklist, 'lr': self.lr, 'errors': errors,
                       'cell': cell}).evaluate()
    if self.want_error:
      self.error = float(np.asarray(expr.sum(errors).glom()).reshape(-1)[0])
    return self

  force = evaluate


def sgd(V, M, U, strata=None, lr=None, want_error=False, dtype=None):
  """One epoch of SGD over the sparse ratings V (users, movies) as an object whose evaluate() / force() runs it,
  updating the factors M (movies, r) and U (users, r) in place.  See the module docstring for the strata, the additions
  and the errors."""
  return NetflixSGD(V, M, U, strata=strata, lr=lr, want_error=want_error, dtype=dtype)
