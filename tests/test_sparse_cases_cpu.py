"""tests/sparse_cases.py checked without a GPU: the term-by-term models against scipy where scipy adds in the same
order, every model inside the derived bound of an accumulation in the next wider type, the structural references
against scipy slicing / reshape / dense assignment -- and the condition that makes the GPU comparisons worth their
bits: on every order-pinning input a plausible WRONG order changes the bits of at least a quarter of the cells or rows
that hold five or more terms, and there are at least twenty of those."""
import numpy as np
import pytest
import scipy.sparse as sps

from tests import sparse_cases as sc

ids = lambda d: np.dtype(d).name        # noqa: E731


def _differing(a, b, which):
  """(fraction of `which` whose bits differ between a and b, how many `which` are)."""
  d = sc.bits(a) != sc.bits(b)
  return float(np.mean(d[which])), int(np.count_nonzero(which))


# ---------------------------------------------------------------------------------------------------- scipy's orders
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
def test_sequential_models_equal_scipy(dtype):
  for family, table in (('whole', sc.planned_whole_lens()), ('long', sc.long_row_lens())):
    for name in table:
      a = sc.matrix(family, name, dtype)
      x = sc.vector(a.shape[1], dtype, 1)
      sc.assert_same_bits(sc.spmv_rows_sequential(a, x), a @ x, (family, name))
  a = sc.spmm_matrix(dtype)
  for n in (2, 65, 259):
    B = sc.real_values(a.shape[1] * n, dtype, 2, n).reshape(a.shape[1], n)
    sc.assert_same_bits(sc.spmm_rows_sequential(a, B), a @ B, n)


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
def test_coo_sum_whole_values_equals_sum_duplicates(dtype):
  for nnz in sc.COO_NNZ[:4]:
    rows, cols, vals = sc.coo_list(nnz, dtype, 'runs', True)
    ref = sps.coo_matrix((vals, (rows, cols)), shape=sc.COO_SHAPE).tocsr()
    ref.sum_duplicates()
    ref.sort_indices()
    indptr, indices, data = sc.coo_sum_list_order(rows, cols, vals, sc.COO_SHAPE)
    np.testing.assert_array_equal(indptr, ref.indptr)
    np.testing.assert_array_equal(indices, ref.indices)
    np.testing.assert_array_equal(data, ref.data)
    # dropped entries: the same as deleting them from the list
    for pattern in sc.DROP_PATTERNS:
      r2 = sc.dropped(rows, pattern)
      keep = r2 >= 0
      ref = sps.coo_matrix((vals[keep], (r2[keep], cols[keep])), shape=sc.COO_SHAPE).tocsr()
      ref.sum_duplicates()
      ref.sort_indices()
      indptr, indices, data = sc.coo_sum_list_order(r2, cols, vals, sc.COO_SHAPE)
      np.testing.assert_array_equal(indptr, ref.indptr)
      np.testing.assert_array_equal(indices, ref.indices)
      np.testing.assert_array_equal(data, ref.data)


def test_spgemm_model_structure_and_whole_values_equal_scipy():
  a = sc.csr_from_lens(sc.fill_lens(3000, 9, 21), 150, np.float64, 21, whole=True)
  lens_b = np.array(sc.fill_lens(1400, 30, 22) + [0] * 150)[:150]
  b = sc.csr_from_lens(lens_b, 90, np.float64, 22, whole=True)
  indptr, indices, data = sc.spgemm_k_ascending(a, b)
  got = sps.csr_matrix((data, indices, indptr), shape=(a.shape[0], 90))
  ref = (a @ b).tocsr()
  np.testing.assert_array_equal(got.toarray(), ref.toarray())
  assert got.has_canonical_format
  assert indptr[-1] >= ref.nnz          # (a cell whose products cancel stays stored)
  _, _, _, offs = sc.spgemm_expand(a, b)
  assert offs[-1] == int(np.diff(b.indptr)[a.indices].sum())


# ---------------------------------------------------------------------------------------------------- derived bound
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
def test_every_spmv_model_is_inside_the_derived_bound(dtype):
  for family, table in (('whole', sc.planned_whole_lens()), ('long', sc.long_row_lens())):
    for name in table:
      a = sc.matrix(family, name, dtype)
      x = sc.vector(a.shape[1], dtype, 1)
      y0 = sc.vector(a.shape[0], dtype, 2)
      for xx, yy in ((x, None), (x, y0), (None, None), (None, y0)):
        sc.check_spmv_bound(sc.spmv_rows_sequential(a, xx, yy), a, xx, yy, (family, name, 'sequential'))
        sc.check_spmv_bound(sc.spmv_chunked(a, xx, yy), a, xx, yy, (family, name, 'chunked'))
  for G in sc.LANES_G:
    a = sc.matrix('lanes', str(G), dtype)
    x = sc.vector(a.shape[1], dtype, 1)
    y0 = sc.vector(a.shape[0], dtype, 2)
    for yy in (None, y0):
      sc.check_spmv_bound(sc.spmv_lanes(a, x, G, yy), a, x, yy, ('lanes', G))


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
def test_coo_and_spmm_models_are_inside_the_derived_bound(dtype):
  wide = sc.WIDER[np.dtype(dtype)]
  eps = sc.EPS[np.dtype(dtype)]
  rows, cols, vals = sc.coo_list(sc.COO_NNZ[2], dtype)
  indptr, indices, data = sc.coo_sum_list_order(rows, cols, vals, sc.COO_SHAPE)
  key = rows.astype(np.int64) * sc.COO_SHAPE[1] + cols
  cells, inv, terms = np.unique(key, return_inverse=True, return_counts=True)
  ref, mag = np.zeros(cells.size, wide), np.zeros(cells.size, wide)
  np.add.at(ref, inv, np.asarray(vals, wide))
  np.add.at(mag, inv, np.abs(np.asarray(vals, wide)))
  assert data.size == cells.size
  assert np.all(np.abs(np.asarray(data, wide) - ref) <= terms * eps * mag)
  a = sc.spmm_matrix(dtype)
  n = 65
  B = sc.real_values(a.shape[1] * n, dtype, 2, n).reshape(a.shape[1], n)
  C0 = sc.real_values(a.shape[0] * n, dtype, 3, n).reshape(a.shape[0], n)
  got = sc.spmm_rows_sequential(a, B, C0)
  dense = np.asarray(a.toarray(), wide)
  ref = np.asarray(C0, wide) + dense @ np.asarray(B, wide)
  mag = np.abs(np.asarray(C0, wide)) + np.abs(dense) @ np.abs(np.asarray(B, wide))
  terms = (np.diff(a.indptr) + 1)[:, None]
  assert np.all(np.abs(np.asarray(got, wide) - ref) <= terms * eps * mag)


# ---------------------------------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('nnz', sc.COO_NNZ)
def test_coo_lists_tell_list_order_from_reversed_order(nnz, dtype):
  rows, cols, vals = sc.coo_list(nnz, dtype)
  terms = sc.coo_cell_terms(rows, cols, sc.COO_SHAPE)
  for want in sc.COO_RUNS:
    assert np.any(terms == want), want
  right = sc.coo_sum_list_order(rows, cols, vals, sc.COO_SHAPE)[2]
  wrong = sc.coo_sum_list_order(rows, cols, vals, sc.COO_SHAPE, reverse=True)[2]
  frac, count = _differing(right, wrong, terms >= 5)
  assert count >= 20 and frac >= 0.25, (frac, count)
  # runs of one and two entries cannot tell
  assert not np.any((sc.bits(right) != sc.bits(wrong))[terms <= 2])


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('shape', [s for s, _ in sc.KEY_WIDTH_SHAPES], ids=lambda s: '%dx%d' % s)
def test_key_width_lists_tell_list_order_from_reversed_order(shape, dtype):
  rows, cols, vals = sc.key_width_list(shape, dtype)
  assert rows.max() == shape[0] - 1 and cols.max() == shape[1] - 1 and rows.min() == 0 and cols.min() == 0
  terms = sc.coo_cell_terms(rows, cols, shape)
  right = sc.coo_sum_list_order(rows, cols, vals, shape)
  wrong = sc.coo_sum_list_order(rows, cols, vals, shape, reverse=True)
  assert right[0][-1] == terms.size and right[0].size == shape[0] + 1
  frac, count = _differing(right[2], wrong[2], terms >= 5)
  assert count >= 20 and frac >= 0.25, (frac, count)


def test_key_width_shapes_sit_on_both_sides_of_every_pass_count():
  assert [sc.key_passes(s) for s, _ in sc.KEY_WIDTH_SHAPES] == [p for _, p in sc.KEY_WIDTH_SHAPES]
  assert sorted(set(p for _, p in sc.KEY_WIDTH_SHAPES)) == [1, 2, 3, 4, 5, 6, 7]
  assert all(s[0] <= 2 ** 20 for s, _ in sc.KEY_WIDTH_SHAPES)


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('name', sc.ORDER_PINNING_LONG)
def test_long_row_matrices_tell_chunked_from_sequential(name, dtype):
  a = sc.matrix('long', name, dtype)
  x = sc.vector(a.shape[1], dtype, 1)
  spanning = np.zeros(a.shape[0], bool)
  spanning[sc.rows_spanning_chunks(a)] = True
  assert np.all(np.diff(a.indptr)[spanning] >= 5)
  for xx in (x, None):
    right, wrong = sc.spmv_chunked(a, xx), sc.spmv_rows_sequential(a, xx)
    frac, count = _differing(right, wrong, spanning)
    assert count >= 20 and frac >= 0.25, (frac, count)
    # a row that lies inside one chunk is summed sequentially by both
    assert not np.any((sc.bits(right) != sc.bits(wrong))[~spanning])


def test_every_long_row_matrix_has_a_spanning_row_and_every_whole_row_matrix_none_over_65():
  for name in sc.long_row_lens():
    a = sc.matrix('long', name, np.float32)
    assert np.diff(a.indptr).max() >= 66 and sc.rows_spanning_chunks(a).size >= 1, name
  for name in sc.planned_whole_lens():
    assert np.diff(sc.matrix('whole', name, np.float32).indptr).max() <= 65, name


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('G', sc.LANES_G)
def test_lanes_matrices_tell_the_lane_tree_from_sequential_and_from_another_width(G, dtype):
  a = sc.matrix('lanes', str(G), dtype)
  x = sc.vector(a.shape[1], dtype, 1)
  lens = np.diff(a.indptr)
  assert set(lens) == {0, 1, G - 1, G, G + 1, 3 * G + 2}
  right = sc.spmv_lanes(a, x, G)
  frac, count = _differing(right, sc.spmv_rows_sequential(a, x), lens >= 5)
  assert count >= 20 and frac >= 0.25, (frac, count)
  # a group width off by a factor of two: rows of up to one term per lane of the smaller width (+ 1: the second term
  # of lane 0 meets the first at the tree's first step) add in the same order and cannot tell -- the forty rows of
  # 3 G + 2 entries can, by a re-association only; five of them telling is asked for
  for other in (G // 2, G * 2):
    if 2 <= other <= 64:
      wrong = sc.spmv_lanes(a, x, other)
      assert not np.any((sc.bits(right) != sc.bits(wrong))[lens <= min(G, other)])
      assert np.count_nonzero((sc.bits(right) != sc.bits(wrong))[lens == 3 * G + 2]) >= 5, other


def test_lanes_stride_matrix_needs_more_than_one_grid_pass():
  a = sc.lanes_stride_matrix(np.float32)
  assert a.shape[0] == 2 ** 21 > sc.GRID_CAP * (256 // 2)
  lens = np.diff(a.indptr)
  assert lens[0] and lens[-1] and lens[2 ** 20] and lens[2 ** 20 - 1] and np.count_nonzero(lens) < 700
  x = sc.vector(a.shape[1], np.float32, 1)
  sc.assert_same_bits(sc.spmv_lanes(a, x, 1), sc.spmv_rows_sequential(a, x))      # one lane IS the sequential order


# ---------------------------------------------------------------------------------------------------- structure
def test_structural_references_against_scipy_and_numpy():
  a = sc.csr_from_lens([0, 0, 3, 0, 7, 1, 0, 0, 5, 0], 40, np.float64, 31)
  coo = a.tocoo()
  np.testing.assert_array_equal(sc.csr_rows_ref(a.indptr, a.nnz), coo.row)
  # box: keep the inside and shift it to the origin == scipy slicing
  for (r0, r1, c0, c1) in ((2, 9, 5, 30), (0, 10, 0, 40), (4, 5, 0, 40), (3, 3, 0, 40)):
    rows, cols = sc.coo_box_ref(coo.row, coo.col, r0, r1, c0, c1, -r0, -c0, 0)
    indptr, indices, data = sc.coo_sum_list_order(rows, cols, coo.data, (r1 - r0, c1 - c0))
    ref = a[r0:r1, c0:c1]
    ref.sort_indices()
    np.testing.assert_array_equal(indptr, ref.indptr)
    np.testing.assert_array_equal(indices, ref.indices)
    np.testing.assert_array_equal(data, ref.data)
    # drop the inside: what is left plus the inside is the whole
    rows2, cols2 = sc.coo_box_ref(coo.row, coo.col, r0, r1, c0, c1, 0, 0, 1)
    assert np.count_nonzero(rows2 >= 0) + np.count_nonzero(rows >= 0) == a.nnz
    np.testing.assert_array_equal(cols2, coo.col)
  # entries dropped on input stay dropped and keep their column
  rows_in = np.array(coo.row)
  rows_in[::4] = -1
  rows, cols = sc.coo_box_ref(rows_in, coo.col, 0, 10, 0, 40, 3, -2, 0)
  assert np.all(rows[::4] == -1) and np.all(cols[::4] == coo.col[::4]) and np.all(rows[1::4] == coo.row[1::4] + 3)
  # reshape == reshape of the dense array; an offset == a window of the flattened array
  dense = a.toarray()
  rows, cols = sc.coo_reshape_ref(coo.row, coo.col, 40, 0, 20, 20)
  got = np.zeros((20, 20))
  got[rows, cols] = coo.data
  np.testing.assert_array_equal(got, dense.reshape(20, 20))
  rows, cols = sc.coo_reshape_ref(coo.row, coo.col, 40, 95, 6, 25)
  keep = rows >= 0
  got = np.zeros((6, 25))
  got[rows[keep], cols[keep]] = coo.data[keep]
  np.testing.assert_array_equal(got, dense.reshape(-1)[95:95 + 150].reshape(6, 25))
  # scatter == dense assignment / addition
  out = sc.real_values(14 * 50, np.float64, 32).reshape(14, 50)
  got, _ = sc.scatter_ref(a, out, 3, 7, 0)
  ref = np.array(out)
  ref[3:13, 7:47][dense != 0] = dense[dense != 0]
  np.testing.assert_array_equal(got, ref)
  got, _ = sc.scatter_ref(a, out, 3, 7, 1)
  ref = np.array(out)
  ref[3:13, 7:47] += dense
  np.testing.assert_array_equal(got, ref)
  mask = (sc._rng(33).rand(14, 60) < 0.5).astype(np.uint8)
  got, gmask = sc.scatter_ref(a, out, 3, 7, 2, mask)
  ref, rmask = np.array(out), np.array(mask)
  for r, c, v in zip(coo.row + 3, coo.col + 7, coo.data):
    ref[r, c] = ref[r, c] + v if rmask[r, c] else v
    rmask[r, c] = 1
  np.testing.assert_array_equal(got, ref)
  np.testing.assert_array_equal(gmask, rmask)


def test_band_matrix_is_canonical_and_leaves_the_named_columns_alone():
  a = sc.band_matrix(32768, 32768, 2 ** 18, (0, 5000, 32767))
  assert a.nnz == 2 ** 18 and a.has_canonical_format and np.diff(a.indptr).max() <= 65
  assert not np.any(np.isin(a.indices, (0, 5000, 32767)))
