"""sp_potrf / sp_trsm_rlt (csrc/linalg.hip) through kernels.py and HipBackend, against the backward error bounds of
tests/linalg_cases.py -- at every order where the code takes another path: below, at and above the LDS block (64) and
the outer block column (256), and 3 * 256 + 17, which spans several outer blocks and ends in a ragged one.

Measured ratios to the bound are printed before each assertion (pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, devarray as D, kernels
from tests import linalg_cases as lc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', lc.ORDERS)
def test_potrf_meets_the_cholesky_bound(be, n, dtype):
  a = lc.spd(n, dtype)
  t = be.from_numpy(a)
  low = be.potrf(t)
  assert low is not t and low.dtype == np.dtype(dtype) and tuple(low.shape) == (n, n)
  got = low.numpy()
  assert t.numpy().tobytes() == a.tobytes()                       # the input is not written
  assert not np.any(np.triu(got, 1))                              # exactly zero above the diagonal
  assert np.all(np.isfinite(got)) and np.all(np.diag(got) > 0)
  ratio = lc.potrf_ratio(a, got)
  print('potrf n=%d %s: ||A - L L^T|| / bound = %.4g' % (n, np.dtype(dtype).name, ratio))
  assert ratio <= 1.0


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', lc.ORDERS)
def test_trsm_rlt_meets_the_substitution_bound(be, n, dtype):
  low = lc.factor(n, dtype)
  lt = be.from_numpy(low)
  for m in lc.ROWS:
    b = lc.rhs(m, n, dtype)
    bt = be.from_numpy(b)
    x = be.trsm_rlt(bt, lt)
    assert x is not bt and x.dtype == np.dtype(dtype) and tuple(x.shape) == (m, n)
    assert bt.numpy().tobytes() == b.tobytes()
    ratio = lc.trsm_ratio(b, low, x.numpy())
    print('trsm_rlt m=%d n=%d %s: ||X L^T - B|| / bound = %.4g' % (m, n, np.dtype(dtype).name, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_trsm_rlt_does_not_read_above_the_diagonal(be, dtype):
  n, m = lc.NB + 1, 37
  low = lc.factor(n, dtype)
  dirty = low + np.triu(np.full((n, n), np.nan, dtype), 1)
  b = be.from_numpy(lc.rhs(m, n, dtype))
  assert be.trsm_rlt(b, be.from_numpy(dirty)).numpy().tobytes() == be.trsm_rlt(b, be.from_numpy(low)).numpy().tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_potrf_reads_the_lower_triangle_only(be, dtype):
  n = lc.OB + 1
  a = lc.spd(n, dtype)
  dirty = np.tril(a) + np.triu(np.full((n, n), np.nan, dtype), 1)
  assert be.potrf(be.from_numpy(dirty)).numpy().tobytes() == be.potrf(be.from_numpy(a)).numpy().tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_views_inside_larger_buffers_keep_their_surroundings(be, dtype):
  n, m = lc.OB + 1, 37
  a, b = lc.spd(n, dtype), lc.rhs(m, n, dtype)
  # A at lda = n + 5, in place
  frame = np.full((n + 2, n + 5), -77.0, dtype)
  frame[1:n + 1, 2:n + 2] = a
  buf = be.from_numpy(frame)
  info = be.zeros((1,), np.int32)
  kernels.potrf(buf[1:n + 1, 2:n + 2], info)
  after = buf.numpy()
  assert int(info.numpy()[0]) == 0
  assert after[1:n + 1, 2:n + 2].tobytes() == be.potrf(be.from_numpy(a)).numpy().tobytes()
  outside = np.ones(frame.shape, bool)
  outside[1:n + 1, 2:n + 2] = False
  assert after[outside].tobytes() == frame[outside].tobytes()
  # the same view through the backend: a new tensor, the buffer untouched
  buf = be.from_numpy(frame)
  low = be.potrf(buf[1:n + 1, 2:n + 2])
  assert buf.numpy().tobytes() == frame.tobytes() and low.numpy().tobytes() == after[1:n + 1, 2:n + 2].tobytes()
  # B at ldb = n + 3, L a view as well
  frame_b = np.full((m + 2, n + 3), -77.0, dtype)
  frame_b[1:m + 1, 3:n + 3] = b
  bbuf = be.from_numpy(frame_b)
  lview = be.from_numpy(after)[1:n + 1, 2:n + 2]
  kernels.trsm_rlt(bbuf[1:m + 1, 3:n + 3], lview)
  after_b = bbuf.numpy()
  outside = np.ones(frame_b.shape, bool)
  outside[1:m + 1, 3:n + 3] = False
  assert after_b[outside].tobytes() == frame_b[outside].tobytes()
  assert lc.trsm_ratio(b, after[1:n + 1, 2:n + 2], after_b[1:m + 1, 3:n + 3]) <= 1.0
  assert after_b[1:m + 1, 3:n + 3].tobytes() == be.trsm_rlt(be.from_numpy(b), lview).numpy().tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_not_positive_definite_names_the_minor_and_returns(be, dtype):
  a = lc.spd(200, dtype).copy()
  a[70, 70] = -1
  t = be.from_numpy(a)
  with pytest.raises(np.linalg.LinAlgError, match=r'\b71-th leading minor'):
    be.potrf(t)
  assert t.numpy().tobytes() == a.tobytes()
  # in place: the flag, and a matrix that is finite everywhere (the kernels behind the pivot did not work on it)
  work, info = be.from_numpy(a), be.zeros((1,), np.int32)
  kernels.potrf(work, info)
  assert int(info.numpy()[0]) == 71 and np.all(np.isfinite(work.numpy()))
  # the backend is whole afterwards
  assert lc.potrf_ratio(lc.spd(65, dtype), be.potrf(be.from_numpy(lc.spd(65, dtype))).numpy()) <= 1.0
  # a NaN on the diagonal is a failed pivot as well, not a NaN-filled factor
  a = lc.spd(200, dtype).copy()
  a[130, 130] = np.nan
  with pytest.raises(np.linalg.LinAlgError, match=r'\b131-th leading minor'):
    be.potrf(be.from_numpy(a))


@pytest.mark.parametrize('dtype', (np.int32, np.float16, np.bool_), ids=lambda d: np.dtype(d).name)
def test_other_dtypes_are_refused(be, dtype):
  sq = be.from_numpy(np.eye(4).astype(dtype))
  with pytest.raises(TypeError, match='astype'):
    be.potrf(sq)
  with pytest.raises(TypeError, match='astype'):
    be.trsm_rlt(sq, sq)
  with pytest.raises(TypeError, match='astype'):
    be.trsm_rlt(be.from_numpy(np.eye(4, dtype=np.float32)), sq)
  x = _hip.extras()
  assert x.sp_potrf(_hip.sp_dtype(dtype), None, 4, 4, None, 0, None, None) != 0
  assert b'astype' in _hip.lib().sp_last_error()
  assert x.sp_trsm_rlt(_hip.sp_dtype(dtype), None, 4, 4, None, 4, 4, None) != 0
  assert b'astype' in _hip.lib().sp_last_error()


def test_shapes_refused_and_empty_operands(be):
  with pytest.raises(ValueError):
    be.potrf(be.from_numpy(np.ones((3, 4), np.float32)))
  with pytest.raises(TypeError, match='astype'):
    be.trsm_rlt(be.from_numpy(np.ones((3, 4), np.float32)), be.from_numpy(np.eye(4)))
  with pytest.raises(ValueError):
    be.trsm_rlt(be.from_numpy(np.ones((3, 5))), be.from_numpy(np.eye(4)))
  for dtype in DTYPES:
    e = be.potrf(D.empty((0, 0), dtype))
    assert tuple(e.shape) == (0, 0) and e.dtype == np.dtype(dtype)
    e = be.trsm_rlt(D.empty((0, 4), dtype), be.from_numpy(np.eye(4, dtype=dtype)))
    assert tuple(e.shape) == (0, 4) and e.dtype == np.dtype(dtype)
    e = be.trsm_rlt(D.empty((5, 0), dtype), D.empty((0, 0), dtype))
    assert tuple(e.shape) == (5, 0)


def test_the_extras_header_lists_the_new_exports():
  from tests.test_abi_cpu import EXTRAS_HEADER, _declared_functions
  assert _declared_functions(EXTRAS_HEADER) == sorted(
      ['sp_sort_rows_workspace_bytes', 'sp_sort_rows', 'sp_potrf_workspace_bytes', 'sp_potrf', 'sp_trsm_rlt'])
  x = _hip.extras()
  for dt in (_hip.SP_F32, _hip.SP_F64):
    assert x.sp_potrf_workspace_bytes(dt, 0) > 0 and x.sp_potrf_workspace_bytes(dt, 64) <= 1024
    # room for the negated, transposed block row of the largest update at n = 3 * 256 + 17: K x N elements, with
    # K = 512 columns to the left of the third block column and N = 256 its width (the last one is 768 x 17)
    assert x.sp_potrf_workspace_bytes(dt, 785) >= 512 * 256 * (4 if dt == _hip.SP_F32 else 8)
