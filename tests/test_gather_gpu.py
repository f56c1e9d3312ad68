"""sp_gather_rows (csrc/update.hip) through kernels.gather_rows against NumPy's `src[idx]`, exact, and `x[idx]`
(expr/filter.py) on HipBackend under the operator cases of tests/gather_cases.py.

The kernel moves words of 16, 4, 2 or 1 bytes -- the widest that the row length, the stride and both base pointers
allow -- so the rows are 1 and 3 bytes (bytes), 2 and 6 (2-byte words), 4, 12 and 2068 (4-byte words), 16 and 48
(16-byte words), and 16-byte rows whose base is 4 bytes or 1 byte past a 16-byte boundary.  4100 indices of 517 words
are 8280 blocks, past the grid's cap of 8192.  The kernel trusts its indices (the range check is eval_index's), so
nothing here hands it an index outside [-n, n): the refusals are tested through the operator only."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import devarray as D
from spartan_amd import kernels
from tests import gather_cases as gc

pytestmark = pytest.mark.gpu


def _gather(src, idx):
  """kernels.gather_rows of a device source and a host index; source and index keep their bytes."""
  before = src.numpy()
  d_idx = D.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))
  out = kernels.gather_rows(src, d_idx)
  got = out.numpy()
  assert src.numpy().tobytes() == before.tobytes() and np.array_equal(d_idx.numpy(), idx)
  return got


def _same(got, want, label):
  assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, got.shape, want.shape)
  assert got.tobytes() == np.ascontiguousarray(want).tobytes(), label


@pytest.mark.parametrize('case', gc.KERNEL_ROWS, ids=lambda c: '%dB' % c[0])
def test_every_word_width(case):
  rb, dtype, row = case
  x = gc.source(gc.N_SRC, dtype, row)
  src = D.from_numpy(x)
  _same(_gather(src, gc.INDEX), x[gc.INDEX], '%d-byte rows' % rb)
  for one in (0, -1, 17):                                   # n_idx == 1
    _same(_gather(src, np.array([one])), x[[one]], '%d-byte rows, index %d' % (rb, one))
  empty = kernels.gather_rows(src, D.empty((0,), np.int64))
  assert tuple(empty.shape) == (0,) + tuple(x.shape[1:])


@pytest.mark.parametrize('case', gc.KERNEL_ROWS, ids=lambda c: '%dB' % c[0])
def test_the_negative_index_of_the_first_row(case):
  rb, dtype, row = case
  x = gc.source(gc.N_SRC, dtype, row)
  idx = np.array([-gc.N_SRC, 3, -gc.N_SRC, gc.N_SRC - 1])
  _same(_gather(D.from_numpy(x), idx), x[idx], '%d-byte rows' % rb)


@pytest.mark.parametrize('shift', (4, 1), ids=('base+4', 'base+1'))
def test_sixteen_byte_rows_on_a_base_that_is_not_sixteen_byte_aligned(shift):
  """A view that starts one element into its buffer: 16-byte rows, but the narrower path must take them."""
  dtype = np.float32 if shift == 4 else np.uint8
  per_row = 16 // np.dtype(dtype).itemsize
  flat = gc.source(1 + gc.N_SRC * per_row, dtype, ())
  buf = D.from_numpy(flat)
  view = buf[1:].reshape(gc.N_SRC, per_row)
  assert view.is_contiguous() and view.data_ptr() % 16 == shift and buf.data_ptr() % 16 == 0
  want = flat[1:].reshape(gc.N_SRC, per_row)
  _same(_gather(view, gc.INDEX), want[gc.INDEX], 'rows of 16 bytes at base + %d' % shift)
  assert buf.numpy().tobytes() == flat.tobytes()


def test_the_grid_strides():
  n_idx, n_src, words = gc.BIG
  x = gc.source(n_src, np.float32, (words,))
  idx = gc.big_index()
  _same(_gather(D.from_numpy(x), idx), x[idx], '%d x %d words' % (n_idx, words))


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize('workers', gc.OP_WORKERS)
def test_operator_on_the_hip_backend(workers):
  ctx = sp.initialize('hip', num_workers=workers)
  try:
    before = ctx.backend.launches
    gc.run_operator_cases(sp, extra_dtypes=(np.int8,))      # (int8: a tile type of this backend alone)
    assert ctx.backend.launches > before
  finally:
    sp.shutdown()


@pytest.mark.parametrize('workers', (1, 3))
def test_an_index_out_of_range_is_an_index_error_on_the_hip_backend(workers):
  ctx = sp.initialize('hip', num_workers=workers)
  try:
    gc.run_range_checks(sp, ctx.backend)
  finally:
    sp.shutdown()
