"""The sparse tile kernels (csrc/sparse.hip, csrc/spmv_blocked.hip) against the term-by-term models and structural
references of tests/sparse_cases.py (proved sound without a GPU by tests/test_sparse_cases_cpu.py).  Real values of
mixed sign and magnitude, and every comparison is on BIT PATTERNS: a sum added in another order fails.

Which order each n == 1 path of sp_csr_spmm guarantees, and the test that pins it:
  planned kernel, longest row <= 65   whole rows in storage order (scipy's csr_matvec order), y0 + s when accumulating
                                      -> test_planned_whole_rows_are_summed_in_storage_order
  planned kernel, longest row >= 66   the row's part in the chunk it starts in sequentially (y0 + s), then one carry per
  stream kernel + fix-up (no plan)    later chunk -- 64 lane-strided partial sums and a shuffle tree -- in chunk order
                                      -> test_long_rows_planned_and_stream_add_chunk_carries_in_chunk_order
  lanes-per-row kernel, G = 2 .. 64   lane g adds entries g, g + G, ...; a shuffle tree over G lanes; y0 + acc
                                      -> test_lanes_per_row_order_for_every_group_width (+ ..._when_the_row_loop_strides)
  blocked kernel (fp32, with a plan)  storage order, like the planned kernel's whole rows
                                      -> test_nonfinite_values_stay_in_their_rows_blocked_kernel (and the existing
                                         tests/test_sparse_kernels_gpu.py::test_spmv_column_blocked_plan_is_bit_identical)
n > 1 starts from C (accumulate) or 0 and adds a * B[k, :] in storage order -> test_spmm_padded_operands_in_storage_order.
sp_coo_to_csr adds equal coordinates in list order -> test_coo_duplicates_are_added_in_list_order; the products of
sparse x sparse meet in k-ascending order -> test_spgemm_adds_products_k_ascending.

Sizes.  The scan behind sp_coo_to_csr works in chunks of 4096: lists of 4095 .. 2 * 4096 + 1 and 70 001 entries.  Key
widths: shapes on both sides of every number of 8-bit radix passes from 1 to 7 (51 bits); 8 passes (more than 56 bits)
would need a tile of more than 2^25 rows, whose row pointers alone are 256 MB -- left out.  n == 1: chunks of 2048 stored
entries, a 64-entry spill behind them, so rows of 64 / 65 / 66 entries starting on entry 2047, rows ending on 2048, rows
of 2049 .. 5000 entries.  The lanes-per-row grid covers 2^20 rows per pass at G = 2: one tile of 2^21 rows.  The blocked
kernel takes tiles from 2^18 entries and 4096 rows on.  n > 1: both sides of the V = 1 / 2 / 4 switches (128, 256) and of
the 64-lane column loop, row lengths around the unroll of 4."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from spartan_amd import _hip
from spartan_amd import devarray as D
from spartan_amd import sparse as S
from spartan_amd._hip import check
from spartan_amd.kernels import _stream, _ws
from tests import sparse_cases as sc

pytestmark = pytest.mark.gpu

ids = lambda d: np.dtype(d).name        # noqa: E731
dev = D.from_numpy


def _p(t):
  return C.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _tile(a):
  """A host CSR matrix as a device tile, arrays as they are (no sort, no compress)."""
  return S.CsrTile(a.shape, a.data.dtype, dev(np.asarray(a.indptr, np.int64)), dev(np.asarray(a.indices, np.int32)),
                   dev(np.ascontiguousarray(a.data)))


def _coo_to_csr(rows, cols, vals, shape):
  """sp_coo_to_csr on host arrays -> (indptr, indices[:kept], data[:kept]) on the host."""
  lib = _hip.lib()
  nnz = int(rows.size)
  r, c, v = dev(np.asarray(rows, np.int32)), dev(np.asarray(cols, np.int32)), dev(np.ascontiguousarray(vals))
  indptr = dev(np.full(shape[0] + 1, -1, np.int64))
  indices, out = dev(np.full(nnz, -1, np.int32)), dev(np.full(nnz, np.nan, vals.dtype))
  ws = _ws.get(lib.sp_coo_to_csr_workspace_bytes(nnz), r.device)
  check(lib.sp_coo_to_csr(_hip.sp_dtype(vals.dtype), shape[0], shape[1], nnz, _p(r), _p(c), _p(v), _p(indptr), _p(indices),
                          _p(out), _p(ws), ws.numel(), _stream()))
  ptr = indptr.numpy()
  kept = int(ptr[-1])
  # the list itself is an input
  np.testing.assert_array_equal(r.numpy(), rows)
  np.testing.assert_array_equal(c.numpy(), cols)
  return ptr, indices.numpy()[:kept], out.numpy()[:kept]


def _check_csr(got, want, label):
  np.testing.assert_array_equal(got[0], want[0], err_msg='%s: indptr' % (label,))
  np.testing.assert_array_equal(got[1], want[1], err_msg='%s: indices' % (label,))
  sc.assert_same_bits(got[2], want[2], label)


def _spmm_raw(A, n, b, ldb, c, ldc, accumulate, plan):
  """sp_csr_spmm as the C-ABI takes it: b / c device arrays (b None: NULL), plan a device array or None."""
  lib = _hip.lib()
  ws = _ws.get(lib.sp_csr_spmm_workspace_bytes(A.nnz, n), A.device)
  check(lib.sp_csr_spmm(_hip.sp_dtype(A.dtype), A.shape[0], A.shape[1], n, A.nnz, _p(A.indptr), _p(A.indices), _p(A.data),
                        _p(b), ldb, _p(c), ldc, 1 if accumulate else 0, _p(plan), _p(ws), ws.numel(), _stream()))


def _spmv(A, x, y0=None, plan=True):
  """y = A x (x None: row sums), or y0 + A x, through sp_csr_spmm with n == 1; a fresh y is prefilled with NaN."""
  m = A.shape[0]
  y = dev(np.full(m, np.nan, A.dtype) if y0 is None else np.ascontiguousarray(y0))
  _spmm_raw(A, 1, None if x is None else dev(np.ascontiguousarray(x)), 1, y, 1, y0 is not None,
            S.spmv_plan(A) if plan else None)
  return y.numpy()


def _all_operands(a, dtype):
  """(x, y0) pairs: with and without a right-hand side (NULL: row sums), with and without accumulate."""
  x = sc.vector(a.shape[1], dtype, 1)
  y0 = sc.vector(a.shape[0], dtype, 2)
  return ((x, None), (x, y0), (None, None), (None, y0))


# ---------------------------------------------------------------------------------------------------- sp_coo_to_csr
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('nnz', sc.COO_NNZ)
def test_coo_duplicates_are_added_in_list_order(nnz, dtype):
  rows, cols, vals = sc.coo_list(nnz, dtype)
  _check_csr(_coo_to_csr(rows, cols, vals, sc.COO_SHAPE), sc.coo_sum_list_order(rows, cols, vals, sc.COO_SHAPE), nnz)


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('kind', ['one_cell', 'distinct'])
def test_coo_one_cell_and_all_distinct(kind, dtype):
  rows, cols, vals = sc.coo_list(sc.COO_NNZ[3], dtype, kind)
  got = _coo_to_csr(rows, cols, vals, sc.COO_SHAPE)
  _check_csr(got, sc.coo_sum_list_order(rows, cols, vals, sc.COO_SHAPE), kind)
  assert got[2].size == (1 if kind == 'one_cell' else rows.size)


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('pattern', sc.DROP_PATTERNS)
def test_coo_dropped_entries(pattern, dtype):
  rows, cols, vals = sc.coo_list(sc.COO_NNZ[2], dtype)
  rows = sc.dropped(rows, pattern)
  got = _coo_to_csr(rows, cols, vals, sc.COO_SHAPE)
  _check_csr(got, sc.coo_sum_list_order(rows, cols, vals, sc.COO_SHAPE), pattern)
  if pattern == 'all':
    assert not got[0].any() and got[1].size == 0


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('shape', [s for s, _ in sc.KEY_WIDTH_SHAPES], ids=lambda s: '%dx%d' % s)
def test_coo_key_widths_one_to_seven_radix_passes(shape, dtype):
  rows, cols, vals = sc.key_width_list(shape, dtype)
  _check_csr(_coo_to_csr(rows, cols, vals, shape), sc.coo_sum_list_order(rows, cols, vals, shape), shape)


# ---------------------------------------------------------------------------------------------------- structure helpers
@pytest.mark.parametrize('nnz', [512, 513])
def test_csr_rows_with_empty_rows(nnz):
  lens = [0, 0] + sc.fill_lens(nnz, 20, nnz) + [0, 0, 0]
  assert 0 in lens[2:-3]
  indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  rows = dev(np.full(nnz, -5, np.int32))
  check(_hip.lib().sp_csr_rows(len(lens), nnz, _p(dev(indptr)), _p(rows), _stream()))
  np.testing.assert_array_equal(rows.numpy(), sc.csr_rows_ref(indptr, nnz))


def _coo_with_dropped(nrows, ncols, nnz, key):
  rng = sc._rng(40, key)
  rows = rng.randint(0, nrows, size=nnz).astype(np.int32)
  cols = rng.randint(0, ncols, size=nnz).astype(np.int32)
  rows[rng.rand(nnz) < 0.2] = -1          # dropped on input: they keep their column whatever it is
  return rows, cols


@pytest.mark.parametrize('drop_inside', [0, 1])
def test_coo_box_edges_shifts_and_dropped_input(drop_inside):
  nrows, ncols = 50, 60
  rows, cols = _coo_with_dropped(nrows, ncols, 1500, 1)
  boxes = ((5, 5, 0, 60), (7, 8, 9, 10), (0, 50, 0, 60), (10, 30, 20, 40), (0, 1, 0, 1), (49, 50, 59, 60))
  for (r0, r1, c0, c1) in boxes:
    for dr, dc in ((0, 0), (3, 4)) + (((-r0, -c0),) if not drop_inside else ((100000, 7),)):
      r, c = dev(rows), dev(cols)
      check(_hip.lib().sp_coo_box(rows.size, _p(r), _p(c), r0, r1, c0, c1, dr, dc, drop_inside, _stream()))
      want = sc.coo_box_ref(rows, cols, r0, r1, c0, c1, dr, dc, drop_inside)
      np.testing.assert_array_equal(r.numpy(), want[0], err_msg=str((r0, r1, c0, c1, dr, dc)))
      np.testing.assert_array_equal(c.numpy(), want[1], err_msg=str((r0, r1, c0, c1, dr, dc)))
      assert np.all(r.numpy()[rows < 0] == -1)


def _reshape(rows, cols, old_cols, offset, new_rows, new_cols):
  r, c = dev(rows), dev(cols)
  check(_hip.lib().sp_coo_reshape(rows.size, _p(r), _p(c), old_cols, offset, new_rows, new_cols, _stream()))
  want = sc.coo_reshape_ref(rows, cols, old_cols, offset, new_rows, new_cols)
  np.testing.assert_array_equal(r.numpy(), want[0])
  np.testing.assert_array_equal(c.numpy(), want[1])
  return want


def test_coo_reshape_offsets_edges_and_dropped_input():
  rows, cols = _coo_with_dropped(40, 50, 1500, 2)
  # linear positions -1, 0, last and last + 1 of a [6, 25] target at offset 95 (and 0, 149, 150 at offset 0)
  edge = np.array([94, 95, 95 + 149, 95 + 150, 0, 149, 150, 40 * 50 - 1])
  rows = np.concatenate([(edge // 50).astype(np.int32), rows])
  cols = np.concatenate([(edge % 50).astype(np.int32), cols])
  want = _reshape(rows, cols, 50, 95, 6, 25)
  assert list(want[0][:4]) == [-1, 0, 5, -1] and list(want[1][1:3]) == [0, 24]
  want = _reshape(rows, cols, 50, 0, 6, 25)
  assert list(want[0][4:7]) == [0, 5, -1]
  _reshape(rows, cols, 50, 0, 100, 20)          # the whole matrix, another split
  _reshape(rows, cols, 50, 1999, 1, 1)          # only the last cell is left


def test_coo_reshape_linear_positions_beyond_2_to_31():
  old = 2 ** 20
  rng = sc._rng(41)
  rows = np.concatenate([[old - 1, old - 1, 0, 2048, -1], rng.randint(old - 4000, old, size=1000)]).astype(np.int32)
  cols = np.concatenate([[old - 1, 0, 0, 1, 77], rng.randint(0, old, size=1000)]).astype(np.int32)
  assert int(rows[0]) * old > 2 ** 31
  want = _reshape(rows, cols, old, 0, 2 ** 10, 2 ** 30)
  assert want[0][0] == 2 ** 10 - 1 and want[1][0] == 2 ** 30 - 1 and want[0][4] == -1 and want[0].max() == 2 ** 10 - 1
  want = _reshape(rows, cols, old, 2 ** 39 + 12345, 2 ** 9, 2 ** 30)     # the second half, shifted
  assert want[0][2] == -1 and want[0][3] == -1 and want[0][0] == 2 ** 9 - 1


# ---------------------------------------------------------------------------------------------------- n == 1
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('name', sorted(sc.planned_whole_lens()))
def test_planned_whole_rows_are_summed_in_storage_order(monkeypatch, name, dtype):
  monkeypatch.setenv('SP_SPMV_ALGO', 'stream')
  a = sc.matrix('whole', name, dtype)
  A = _tile(a)
  plan = S.spmv_plan(A).numpy()
  assert plan[-2] == np.diff(a.indptr).max() <= sc.SPMV_SPILL + 1       # the longest row: the whole-row mode
  for x, y0 in _all_operands(a, dtype):
    sc.assert_same_bits(_spmv(A, x, y0), sc.spmv_rows_sequential(a, x, y0), (name, x is None, y0 is None))


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('name', sorted(sc.long_row_lens()))
def test_long_rows_planned_and_stream_add_chunk_carries_in_chunk_order(monkeypatch, name, dtype):
  monkeypatch.setenv('SP_SPMV_ALGO', 'stream')
  a = sc.matrix('long', name, dtype)
  A = _tile(a)
  assert S.spmv_plan(A).numpy()[-2] == np.diff(a.indptr).max() >= sc.SPMV_SPILL + 2
  for x, y0 in _all_operands(a, dtype):
    want = sc.spmv_chunked(a, x, y0)
    label = (name, x is None, y0 is None)
    sc.assert_same_bits(_spmv(A, x, y0, plan=True), want, label + ('planned',))
    # a second launch on the same plan: the arrival counter was reset
    sc.assert_same_bits(_spmv(A, x, y0, plan=True), want, label + ('planned again',))
    assert S.spmv_plan(A).numpy()[-1] == 0
    sc.assert_same_bits(_spmv(A, x, y0, plan=False), want, label + ('stream + fix-up',))


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('name', ['row65_starts_at_2047', 'nnz_2049'])
def test_stream_kernel_without_a_plan_carries_short_rows_too(monkeypatch, name, dtype):
  """Without a plan nothing knows the longest row: the stream kernel cuts every row at the chunk's end."""
  monkeypatch.setenv('SP_SPMV_ALGO', 'stream')
  a = sc.matrix('whole', name, dtype)
  for x, y0 in _all_operands(a, dtype):
    sc.assert_same_bits(_spmv(_tile(a), x, y0, plan=False), sc.spmv_chunked(a, x, y0), (name, x is None, y0 is None))


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('G', sc.LANES_G)
def test_lanes_per_row_order_for_every_group_width(monkeypatch, G, dtype):
  monkeypatch.setenv('SP_SPMV_ALGO', 'vector')
  monkeypatch.setenv('SP_SPMV_G', str(G))
  a = sc.matrix('lanes', str(G), dtype)
  A = _tile(a)
  for x, y0 in _all_operands(a, dtype):
    sc.assert_same_bits(_spmv(A, x, y0, plan=False), sc.spmv_lanes(a, x, G, y0), (G, x is None, y0 is None))


@pytest.mark.parametrize('G', [2, 64])
def test_lanes_per_row_order_when_the_row_loop_strides(monkeypatch, G):
  monkeypatch.setenv('SP_SPMV_ALGO', 'vector')
  monkeypatch.setenv('SP_SPMV_G', str(G))
  a = sc.lanes_stride_matrix(np.float32)
  assert a.shape[0] > sc.GRID_CAP * (256 // G)
  A = _tile(a)
  x = sc.vector(a.shape[1], np.float32, 1)
  sc.assert_same_bits(_spmv(A, x, None, plan=False), sc.spmv_lanes(a, x, G))
  y0 = sc.vector(a.shape[0], np.float32, 2)
  sc.assert_same_bits(_spmv(A, x, y0, plan=False), sc.spmv_lanes(a, x, G, y0))


# ---------------------------------------------------------------------------------------------------- non-finite values
def _rows_with_nan(y, m):
  return np.isnan(np.asarray(y)).reshape(m, -1).any(axis=1)


def _nonfinite_locality(run, model, a, dtype, n=None):
  """run(a, x) -> y on one kernel path, model(a, x) its term-by-term model; x is [k] (n None) or [k, n].
  (a) NaN / +-Inf in x where no entry refers to -- column 0 and the last among them -- change nothing;
  (b) NaN at two referenced columns: NaN in exactly the model's rows, every other row keeps its bits;
  (c) a stored Inf against x = 0 and a stored explicit 0 against x = Inf: NaN in those two rows only."""
  m, k = a.shape
  unref = list(sc.unreferenced(k))
  assert not np.any(np.isin(a.indices, unref))
  x = np.array(sc.real_values(k * (n or 1), dtype, 50).reshape((k,) if n is None else (k, n)))
  x[unref] = 0
  clean = run(a, x)
  sc.assert_same_bits(clean, model(a, x), 'clean')
  assert np.all(np.isfinite(clean))
  xa = np.array(x)
  xa[unref[0]], xa[unref[1]], xa[unref[2]] = np.nan, np.inf, -np.inf
  sc.assert_same_bits(run(a, xa), clean, '(a) unreferenced columns')
  xb = np.array(x)
  cols_b = [int(a.indices[0]), int(a.indices[a.nnz // 2])]
  xb[cols_b] = np.nan
  got, want = run(a, xb), model(a, xb)
  hit = _rows_with_nan(want, m)
  assert 1 <= np.count_nonzero(hit) < m and np.array_equal(hit, np.isin(np.arange(m), sc.csr_rows_ref(a.indptr, a.nnz)[np.isin(a.indices, cols_b)]))
  sc.assert_same_bits_nan_aware(got, want, '(b) NaN in referenced columns')
  sc.assert_same_bits(got.reshape(m, -1)[~hit], clean.reshape(m, -1)[~hit], '(b) other rows')
  lens = np.diff(a.indptr)
  r1, r2 = int(np.nonzero(lens >= 2)[0][0]), int(np.nonzero(lens >= 2)[0][-1])
  e1, e2 = int(a.indptr[r1]), int(a.indptr[r2]) + 1
  assert r1 != r2 and a.indices[e1] != a.indices[e2]
  data = np.array(a.data)
  data[e1], data[e2] = np.inf, 0
  xc = np.array(x)
  xc[a.indices[e1]], xc[a.indices[e2]] = 0, np.inf
  a2 = sps.csr_matrix((data, a.indices, a.indptr), shape=a.shape)
  got, want = run(a2, xc), model(a2, xc)
  sc.assert_same_bits_nan_aware(got, want, '(c) Inf * 0 and 0 * Inf')
  assert sorted(np.nonzero(_rows_with_nan(got, m))[0]) == sorted({r1, r2})


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('path', ['planned whole rows', 'planned long rows', 'stream', 'lanes'])
def test_nonfinite_values_stay_in_their_rows_n1(monkeypatch, path, dtype):
  monkeypatch.setenv('SP_SPMV_ALGO', 'vector' if path == 'lanes' else 'stream')
  if path == 'lanes':
    monkeypatch.setenv('SP_SPMV_G', '8')
    a, model = sc.matrix('lanes', '8', dtype), lambda a, x: sc.spmv_lanes(a, x, 8)
  elif path == 'planned whole rows':
    # nnz is no multiple of 2048: the last chunk's lanes past nnz hold v = 0, col = 0 and multiply x[0]
    a, model = sc.matrix('whole', 'row65_starts_at_2047', dtype), sc.spmv_rows_sequential
  else:
    a, model = sc.matrix('long', 'row65_starts_at_2047_and_66', dtype), sc.spmv_chunked
  assert a.nnz % sc.SPMV_CH != 0
  _nonfinite_locality(lambda a, x: _spmv(_tile(a), x, None, plan=path.startswith('planned')), model, a, dtype)


@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('n', [5, 130, 260], ids=['V1', 'V2', 'V4'])
def test_nonfinite_values_stay_in_their_rows_spmm(n, dtype):
  def run(a, B):
    c = dev(np.full((a.shape[0], n), np.nan, dtype))
    _spmm_raw(_tile(a), n, dev(B), n, c, n, False, None)
    return c.numpy()
  _nonfinite_locality(run, sc.spmm_rows_sequential, sc.spmm_matrix(dtype), dtype, n)


@pytest.mark.parametrize('k', [32768, 30000], ids=['square', 'narrower_last_slice'])
def test_nonfinite_values_stay_in_their_rows_blocked_kernel(k):
  m, nnz = 32768, 2 ** 18                   # the smallest tile that gets a blocked plan
  unref = sc.unreferenced(k)
  a = sc.band_matrix(m, k, nnz, unref)
  A = _tile(a)
  plan = S.spmv_block_plan(A)
  assert plan is not False
  staged = sc.staged_segments(plan.numpy())
  # every planted column lies in a slice that some row block stages through LDS; the last slice is narrower
  for c in unref:
    assert any(lo <= c < lo + w for lo, w in staged), (c, staged)
  assert any(w < sc.BSP_S and lo + w == k for lo, w in staged)

  def run(a, x):
    t = _tile(a)
    assert S.spmv_block_plan(t) is not False
    return S.spmm(t, dev(np.ascontiguousarray(x))).numpy()
  _nonfinite_locality(run, sc.spmv_rows_sequential, a, np.float32)
  # one entry fewer: no plan
  assert S.spmv_block_plan(_tile(sc.band_matrix(m, k, nnz - 1, unref))) is False


# ---------------------------------------------------------------------------------------------------- n > 1
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('n', sc.SPMM_N)
def test_spmm_padded_operands_in_storage_order(n, dtype):
  a = sc.spmm_matrix(dtype)
  A = _tile(a)
  m, k = a.shape
  ldb, ldc = n + 3, n + 5
  B = np.full((k, ldb), np.nan, dtype)        # the padding of B is never read
  B[:, :n] = sc.real_values(k * n, dtype, 60, n).reshape(k, n)
  C0 = np.full((m, ldc), 12345.0, dtype)      # the padding of C comes back untouched
  C0[:, :n] = sc.real_values(m * n, dtype, 61, n).reshape(m, n)
  for accumulate in (False, True):
    start = np.array(C0)
    if not accumulate:
      start[:, :n] = np.nan                   # assignment does not read C
    c = dev(start)
    _spmm_raw(A, n, dev(B), ldb, c, ldc, accumulate, None)
    got = c.numpy()
    want = sc.spmm_rows_sequential(a, B[:, :n], C0[:, :n] if accumulate else None)
    sc.assert_same_bits(np.ascontiguousarray(got[:, :n]), want, (n, accumulate))
    sc.assert_same_bits(np.ascontiguousarray(got[:, n:]), np.ascontiguousarray(C0[:, n:]), (n, accumulate, 'padding'))


# ---------------------------------------------------------------------------------------------------- sp_csr_scatter
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
def test_scatter_offsets_leading_dimensions_and_mask(dtype):
  a = sc.csr_from_lens([0, 0, 5, 0, 0, 9, 1, 40, 0, 3, 0, 0], 45, dtype, 70)
  A = _tile(a)
  rows_out, ld, ldmask, row0, col0 = 20, 64, 71, 5, 13
  base = sc.real_values(rows_out * ld, dtype, 71).reshape(rows_out, ld)
  mask0 = (sc._rng(72).rand(rows_out, ldmask) < 0.5).astype(np.uint8)
  for mode in (0, 1, 2):
    start = np.array(base)
    if mode == 0:
      start[row0:row0 + a.shape[0], col0:col0 + a.shape[1]][a.toarray() != 0] = np.nan      # assign does not read
    out, mask = dev(start), dev(mask0)
    check(_hip.lib().sp_csr_scatter(_hip.sp_dtype(dtype), a.shape[0], a.nnz, _p(A.indptr), _p(A.indices), _p(A.data), _p(out),
                                    ld, row0, col0, _p(mask) if mode == 2 else C.c_void_p(0), ldmask, mode, _stream()))
    want, wmask = sc.scatter_ref(a, start, row0, col0, mode, mask0 if mode == 2 else None)
    assert np.all(np.isfinite(want))
    sc.assert_same_bits(out.numpy(), want, mode)          # the written cells AND every cell around them
    np.testing.assert_array_equal(mask.numpy(), wmask if mode == 2 else mask0)


# ---------------------------------------------------------------------------------------------------- sparse x sparse
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
@pytest.mark.parametrize('nnz_a', [4095, 4096, 4097])
def test_spgemm_adds_products_k_ascending(nnz_a, dtype):
  a = sc.csr_from_lens(sc.fill_lens(nnz_a, 40, nnz_a), 150, dtype, 80)
  lens_b = np.array(sc.fill_lens(4000, 60, 81) + [0] * 150)[:150]       # B has empty rows that A refers to
  b = sc.csr_from_lens(lens_b, 90, dtype, 81)
  assert np.any(lens_b[a.indices] == 0)
  A, B = _tile(a), _tile(b)
  rows, cols, vals, offs = sc.spgemm_expand(a, b)
  lib = _hip.lib()
  d_offs, d_total = dev(np.full(nnz_a + 1, -1, np.int32)), dev(np.full(1, -1, np.int64))
  ws = _ws.get(lib.sp_spgemm_count_workspace_bytes(nnz_a), A.device)
  check(lib.sp_spgemm_count(nnz_a, _p(A.indices), _p(B.indptr), _p(d_offs), _p(d_total), _p(ws), ws.numel(), _stream()))
  np.testing.assert_array_equal(d_offs.numpy(), offs)
  assert int(d_total.numpy()[0]) == int(offs[-1]) == rows.size
  d_rows, d_cols, d_vals = dev(np.full(rows.size, -1, np.int32)), dev(np.full(rows.size, -1, np.int32)), dev(np.full(rows.size, np.nan, dtype))
  check(lib.sp_spgemm_expand(_hip.sp_dtype(dtype), a.shape[0], nnz_a, _p(A.indptr), _p(A.indices), _p(A.data), _p(B.indptr),
                             _p(B.indices), _p(B.data), _p(d_offs), _p(d_rows), _p(d_cols), _p(d_vals), _stream()))
  np.testing.assert_array_equal(d_rows.numpy(), rows)
  np.testing.assert_array_equal(d_cols.numpy(), cols)
  sc.assert_same_bits(d_vals.numpy(), vals, 'products')
  want = sc.spgemm_k_ascending(a, b)
  terms = sc.coo_cell_terms(rows, cols, (a.shape[0], 90))
  assert np.count_nonzero(terms >= 5) >= 20
  got = S.spgemm(A, B)
  _check_csr((got.indptr.numpy(), got.indices.numpy(), got.data.numpy()), want, nnz_a)
