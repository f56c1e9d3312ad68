"""Item-based collaborative filtering (interface of the reference's spartan/examples/cf/item_recommender.py:
`ItemBasedRecommender(rating_table, k).precompute()` sets `top_k_similar_table` and `top_k_similar_indices`, both (N, k);
its tests/test_item_recommender.py runs a csr sparse_rand table of 8000 users x 800 items).

The rating table is [users, items]; the similarity of two items is the cosine of their columns,

    sim(j, i) = nan_to_num( r[:, j] . r[:, i] / (|r[:, j]| |r[:, i]|) )

so an item nobody rated (norm 0) has similarity 0 with every item, itself included, and an item is NOT excluded from
its own list (the reference keeps it; its similarity with itself is 1 up to rounding).

  'fused' (the default)  the reference's structure without its N x N table.  The item norms are the reference's
             expression sqrt(sum(r * r, axis=0)) on the map and reduce kernels for a dense table.  For a SPARSE table
             that expression does not evaluate on every backend here (on host tiles `multiply` of two scipy matrices
             is their matrix product), so its norms are computed per densified band, in a shuffle of their own over
             the bands, by the same expression on the band.  The work is ONE shuffle over the column bands
             of divup(N, num_workers) items (the reference's calc_tile_hint(axis=1); a dense table is retiled into
             them, a sparse table is read in place: retiling would make it dense).  A band's tile body fetches its
             [users, band] columns and walks all N items in steps of divup(N, num_workers) columns, exactly as the
             reference's _similarity_mapper does; every step is one _cf.item_topk call (HipBackend: sp_item_topk --
             similarity and top-k in one pass) with index_offset = the step's first column, pasted into one slot of a
             [band, steps * k] candidate pair, and one _cf.item_topk_merge follows the steps.  A table of one band
             needs one call and no merge.  Sparse bands and steps are densified on the device per step
             (sparse_to_dense): the only dense storage is users x (band + step); nothing of size N x N or users x N
             is made for a sparse table.
  'table'    the reference as written, for comparison and as the benchmark's yardstick: `similarity_table` (N x N,
             distributed) = dot(r^T, r) / (norm norm^T) with nan_to_num on the map kernels, then the k best of every row
             through `argsort` / `sort` of the negated table.  Only this method sets the `similarity_table` attribute.
             A sparse table is made dense for it.

Deviations from the reference:
  * Every row of the two results is ordered by (similarity descending, index ascending).  The reference leaves a row
    in the order its quick-select (helper.pyx argpartsort) stops in, which is arbitrary; the ordering is an addition.
  * `method` and `dtype` are additions.  float32 and float64 tables are kept, every other dtype is converted to
    float64; dtype= forces one of the two.  top_k_similar_indices is int64.
  * k > N raises ValueError with the reference's assertion message (the reference asserts); k < 1 or k > 128 (the
    kernel's list length), a table that is not 2-D and an unknown method raise ValueError."""
import numpy as np

from ... import context, expr, util
from ...array import distarray, extent, tile as tile_mod
from . import _cf

METHODS = ('fused', 'table')
_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _dense(be, t, dtype):
  """A fetched piece of the table as a dense tile."""
  if isinstance(t, distarray.Absent):
    return t
  if tile_mod.is_sparse_blob(t):
    return be.sparse_to_dense(be.sparse_blob(t, dtype))
  if isinstance(t, tile_mod.EmptyBlob):
    return be.zeros(t.shape, dtype)
  return t


def _norm_mapper(array, ex, table=None, norms=None):
  """Tile body of the norm pass over a SPARSE table: the reference's sqrt(sum(r * r, axis=0)) on this band of items,
  densified."""
  be = context.get().backend
  users = table.shape[0]
  band = _dense(be, table.fetch(extent.create((0, ex.ul[0]), (users, ex.lr[0]), table.shape)), np.dtype(table.dtype))
  if not isinstance(band, distarray.Absent):
    band = np.sqrt((band * band).sum(axis=0))          # (a device tile's operators are the map and reduce kernels)
  norms.update(ex, band)
  return []


_norm_mapper.yields_fresh_tensors = True


def _topk_mapper(array, ex, table=None, k=None, step=None, top_sim=None, top_idx=None):
  """Tile body of the shuffle over the bands of the item norms: the k most similar items of this band's items among
  all N, into the band's rows of the two (N, k) targets."""
  be = context.get().backend
  lo, hi = ex.ul[0], ex.lr[0]
  users, n = table.shape
  dtype = np.dtype(table.dtype)
  targets = _dense(be, table.fetch(extent.create((0, lo), (users, hi), table.shape)), dtype)
  tnorm = array.fetch(ex)
  starts = list(range(0, n, step))
  absent = isinstance(targets, distarray.Absent)
  cand_sim = cand_idx = None
  if len(starts) > 1 and not absent:
    cand_sim, cand_idx = be.empty((hi - lo, len(starts) * k), dtype), be.empty((hi - lo, len(starts) * k), np.int64)
  sim = idx = None
  for slot, first in enumerate(starts):
    last = min(first + step, n)
    sources = _dense(be, table.fetch(extent.create((0, first), (users, last), table.shape)), dtype)
    snorm = array.fetch(extent.create((first,), (last,), (n,)))
    sim, idx = _cf.item_topk(targets, tnorm, sources, snorm, k, index_offset=first)
    if cand_sim is not None:
      where = (slice(0, hi - lo), slice(slot * k, (slot + 1) * k))
      be.paste(cand_sim, where, sim)
      be.paste(cand_idx, where, idx)
  if cand_sim is not None:
    sim, idx = _cf.item_topk_merge(cand_sim, cand_idx, k)
  where = extent.create((lo, 0), (hi, k), (n, k))
  top_sim.update(where, sim)
  top_idx.update(where, idx)
  return []


_topk_mapper.yields_fresh_tensors = True      # the kernel's output (or NumPy's), never a fetched tile


def _order_rows(sim, idx):
  """Host rows re-ordered by (similarity descending, index ascending)."""
  order = np.lexsort((idx, -sim), axis=1)
  return (np.ascontiguousarray(np.take_along_axis(sim, order, axis=1)),
          np.ascontiguousarray(np.take_along_axis(idx, order, axis=1)))


class ItemBasedRecommender(object):
  """rating_table: expression / distributed array (dense or sparse) / NumPy array / scipy.sparse matrix of shape (N_USERS, N_ITEMS);
  k: how many most similar items are found for every item, 1 <= k <= min(N_ITEMS, 128); method: 'fused' | 'table';
  dtype: None (float32 and float64 tables are kept, others become float64), np.float32 or np.float64."""

  def __init__(self, rating_table, k=10, method='fused', dtype=None):
    if method not in METHODS:
      raise ValueError('ItemBasedRecommender: unknown method %r (%s)' % (method, ' '.join(METHODS)))
    if isinstance(rating_table, np.ndarray) or tile_mod.is_sparse_blob(rating_table):      # (scipy.sparse: a sparse array)
      rating_table = expr.from_numpy(rating_table)
    if len(rating_table.shape) != 2:
      raise ValueError('ItemBasedRecommender: expected a rating table of shape (users, items), got %s'
                       % (tuple(rating_table.shape),))
    users, n = (int(v) for v in rating_table.shape)
    # (k through the kernels' one copy of the refusals; the dtype is settled below)
    k = _cf.check_operands([np.float64] * 4, (users, n), (n,), (users, n), (n,), k, what='ItemBasedRecommender')[4]
    if rating_table.shape[1] < k:
      raise ValueError('The number of items must be grater or equal than k!')
    if dtype is not None and np.dtype(dtype) not in _FLOATS:
      raise ValueError('ItemBasedRecommender: dtype %s (float32 float64)' % (np.dtype(dtype),))
    table = expr.evaluate(rating_table)
    want = np.dtype(dtype) if dtype is not None else np.dtype(table.dtype)
    if want not in _FLOATS:
      want = np.dtype(np.float64)
    if np.dtype(table.dtype) != want:
      table = expr.evaluate(expr.astype(table, want))
    self.sparse = bool(getattr(table, 'sparse', False))
    band = util.divup(int(table.shape[1]), context.get().num_workers)
    if not self.sparse:          # (the reference: expr.retile(rating_table, calc_tile_hint(rating_table, axis=1)))
      table = expr.evaluate(expr.retile(table, tile_hint=(max(int(table.shape[0]), 1), max(band, 1))))
    self.rating_table = table
    self.k = k
    self.method = method
    self.dtype = want

  def _get_norm_of_each_item(self, rating_table):
    """item_norm[i] = || rating_table[:, i] ||, shape (N,): the reference's expression."""
    return expr.sqrt(expr.sum(expr.multiply(rating_table, rating_table), axis=0))

  def precompute(self):
    """Sets top_k_similar_table (N, k), the similarities of the k most similar items of every item, best first, and
    top_k_similar_indices (N, k) int64, their item numbers; both host arrays."""
    if self.method == 'fused':
      sim, idx = self._fused()
    else:
      sim, idx = self._table()
    self.top_k_similar_table = sim
    self.top_k_similar_indices = idx

  def _norms(self, step):
    """The item norms as an evaluated (N,) array in bands of `step` items."""
    table = self.rating_table
    n = int(table.shape[1])
    if not self.sparse:
      return expr.evaluate(expr.retile(expr.astype(self._get_norm_of_each_item(table), self.dtype), tile_hint=(step,)))
    norms = expr.ndarray((n,), dtype=self.dtype, tile_hint=(step,))
    expr.shuffle(norms, _norm_mapper, kw={'table': table, 'norms': norms}, shape_hint=(1,)).evaluate()
    return expr.evaluate(norms)

  def _fused(self):
    table, k = self.rating_table, self.k
    n = int(table.shape[1])
    step = max(util.divup(n, context.get().num_workers), 1)
    norms = self._norms(step)
    top_sim = expr.ndarray((n, k), dtype=self.dtype, tile_hint=(step, k))
    top_idx = expr.ndarray((n, k), dtype=np.int64, tile_hint=(step, k))
    expr.shuffle(norms, _topk_mapper, kw={'table': table, 'k': k, 'step': step, 'top_sim': top_sim, 'top_idx': top_idx},
                 shape_hint=(1,)).evaluate()
    sim, idx = np.asarray(top_sim.glom()), np.asarray(top_idx.glom())
    return np.ascontiguousarray(sim), np.ascontiguousarray(idx.astype(np.int64, copy=False))

  def _table(self):
    table, k, dt = self.rating_table, self.k, self.dtype
    n = int(table.shape[1])
    dense = table
    if self.sparse:              # (the Gram matrix below is the dense GEMM)
      dense = expr.from_numpy(np.asarray(expr.lazify(table).glom().todense(), dtype=dt))
    norm = self._get_norm_of_each_item(dense).evaluate()
    dots = expr.dot(expr.transpose(dense), dense)
    norms = expr.reshape(norm, (n, 1)) * expr.reshape(norm, (1, n))
    q = dots / norms
    # np.nan_to_num on the map kernels: NaN -> 0, then the infinities onto the largest finite values
    q = expr.map((expr.equal(q, q), q, dt.type(0)), fn=np.where)
    q = expr.minimum(expr.maximum(q, np.finfo(dt).min), np.finfo(dt).max)
    self.similarity_table = expr.evaluate(expr.astype(q, dt))
    from ... import argsort, sort          # (the sort family resolves on first use, not with the package)
    flipped = expr.lazify(self.similarity_table) * dt.type(-1)
    idx = np.asarray(argsort(flipped, axis=1)[:, :k].optimized().glom()).astype(np.int64)
    sim = -np.asarray(sort(flipped, axis=1)[:, :k].optimized().glom()).astype(dt, copy=False)
    return _order_rows(sim, idx)
