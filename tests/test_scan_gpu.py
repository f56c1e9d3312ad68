"""sp_cumscan (csrc/update.hip) through kernels.cumscan, and the scan operator on HipBackend, against the references
and derived bounds of tests/scan_cases.py (proved sound without a GPU by tests/test_scan_cases_cpu.py).

Shapes.  The row kernel (inner == 1) scans 64 elements per step with a carry from lane 63 and puts 4 lines into a
block: A is 1, 2 and both sides of 64 and 128, then 1000; outer is 1 and both sides of 4; (16384 + 5) x 70 has more
lines than the capped grid has waves, so the line loop strides.  The column kernel (inner > 1) has one thread per line
in blocks of 256: outer x inner is on both sides of 256 and of 768.  Nothing is larger than 16389 x 70.  Measured
figures are printed before each assertion (pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import devarray as D
from spartan_amd import kernels
from tests import scan_cases as sc

pytestmark = pytest.mark.gpu

ids = lambda d: np.dtype(d).name        # noqa: E731
OPS = (False, True)
op_ids = lambda p: 'prod' if p else 'sum'        # noqa: E731


def _scan(x, axis, product):
  """kernels.cumscan on a host array: the result on the host; the input on the device keeps its bytes."""
  src = D.from_numpy(np.ascontiguousarray(x))
  out = D.empty(tuple(x.shape), x.dtype)
  assert kernels.cumscan(src, out, axis, product) is out
  assert src.numpy().tobytes() == np.ascontiguousarray(x).tobytes()
  return out.numpy()


def _check(x, product, label):
  """One [outer, A, inner] case: integers exact; floats bit-equal to NumPy's order in the column kernel, within the
  derived bound of the wide reference in the row kernel."""
  got = _scan(x, 1, product)
  if np.dtype(x.dtype).kind != 'f' or x.shape[2] > 1:
    sc.check_exact(got, sc.numpy_scan(x, 1, product), label)
  else:
    sc.check_float(got, x, 1, product, label)


@pytest.mark.parametrize('product', OPS, ids=op_ids)
@pytest.mark.parametrize('dtype', sc.DTYPES, ids=ids)
def test_row_kernel(dtype, product):
  for shape in sc.ROW_SHAPES:
    label = 'rows %s %s %s' % (shape, np.dtype(dtype).name, op_ids(product))
    _check(sc.data(shape, dtype, product), product, label)
    if np.dtype(dtype).kind == 'f':
      # whole values whose every partial result is representable: exact in any order
      x = sc.data(shape, dtype, product, 'whole')
      sc.check_exact(_scan(x, 1, product), sc.numpy_scan(x, 1, product), label + ' whole')


@pytest.mark.parametrize('product', OPS, ids=op_ids)
@pytest.mark.parametrize('dtype', sc.DTYPES, ids=ids)
def test_row_kernel_line_loop_strides(dtype, product):
  _check(sc.data(sc.ROW_STRIDE_SHAPE, dtype, product), product,
         'rows %s %s %s' % (sc.ROW_STRIDE_SHAPE, np.dtype(dtype).name, op_ids(product)))


@pytest.mark.parametrize('product', OPS, ids=op_ids)
@pytest.mark.parametrize('dtype', sc.DTYPES, ids=ids)
def test_column_kernel(dtype, product):
  for shape in sc.COL_SHAPES + (sc.MIDDLE_AXIS_SHAPE,):
    _check(sc.data(shape, dtype, product), product, 'columns %s %s %s' % (shape, np.dtype(dtype).name, op_ids(product)))
  # a 3-D tile along its middle axis, and the same tile along its last (rows) and first (columns) axes
  x = sc.data(sc.MIDDLE_AXIS_SHAPE, dtype, product)
  sc.check_exact(_scan(x, 0, product), sc.numpy_scan(x, 0, product), 'axis 0 of 3-D')
  if np.dtype(dtype).kind != 'f':
    sc.check_exact(_scan(x, 2, product), sc.numpy_scan(x, 2, product), 'axis 2 of 3-D')
  else:
    sc.check_float(_scan(x, 2, product), x, 2, product, 'axis 2 of 3-D')


@pytest.mark.parametrize('inner', (1, 3), ids=('rows', 'columns'))
@pytest.mark.parametrize('product', OPS, ids=op_ids)
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
def test_nan_inf_and_zero_inside_a_chunk_and_on_its_boundary(dtype, product, inner):
  clean, planted, plans = sc.edge_lines(dtype, product, inner)
  label = '%s %s %s' % (np.dtype(dtype).name, op_ids(product), 'rows' if inner == 1 else 'columns')
  got_clean, got_planted = _scan(clean, 1, product), _scan(planted, 1, product)
  sc.check_edges(got_clean, got_planted, plans, label)
  if inner > 1:
    np.testing.assert_array_equal(got_planted, sc.numpy_scan(planted, 1, product))     # (NaN == NaN here)
  if product:
    x = sc.overflow_lines(dtype, inner)
    sc.check_exact(_scan(x, 1, True), sc.numpy_scan(x, 1, True), label + ' overflow to inf')


def test_refusals_and_empty_tiles():
  for shape in ((0, 5), (5, 0)):
    out = D.empty(shape, np.float32)
    kernels.cumscan(D.from_numpy(np.zeros(shape, np.float32)), out, 1)
    assert tuple(out.shape) == shape
  src = D.from_numpy(np.zeros((4, 4), np.uint8))
  with pytest.raises(Exception, match='unsupported dtype'):
    kernels.cumscan(src, D.empty((4, 4), np.uint8), 1)


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize('dtype', sc.OP_DTYPES, ids=ids)
@pytest.mark.parametrize('workers', sc.OP_WORKERS)
def test_operator_on_the_hip_backend(workers, dtype):
  ctx = sp.initialize('hip', num_workers=workers)
  try:
    before = ctx.backend.launches
    sc.run_operator_cases(sp, workers, dtype)
    assert ctx.backend.launches > before
  finally:
    sp.shutdown()


def test_operator_refusals_on_the_hip_backend():
  ctx = sp.initialize('hip', num_workers=3)
  try:
    sc.run_refusals(sp, ctx.backend)
  finally:
    sp.shutdown()
