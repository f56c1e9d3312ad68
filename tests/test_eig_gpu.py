"""sp_syevj (csrc/linalg.hip) through kernels.py and HipBackend.syev, against the yardsticks of tests/eig_cases.py: at
most MARGIN = 4 times the ratios of the NumPy transcription of the same scheme on the same input and dtype.

Orders: 1, 2, 3 (an odd order: one index sits each round out), 63, 64, 65 (both sides of the limit of the path that
keeps A and V in LDS: 64 in float32, 63 in float64), 130 and 257 (the path of one launch per round; 257 is odd and
spans several tiles with a ragged last one).  All four kinds of input at 65 and 257, `indef` elsewhere.

Every ratio is printed next to its limit before it is asserted (pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, devarray as D, kernels
from tests import eig_cases as ec

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
CASES = [('indef', n) for n in (1, 2, 3, 63, 64, 130)] + [(kind, n) for n in (65, 257) for kind in ec.KINDS]


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _solve(be, a):
  w, v = be.syev(be.from_numpy(a))
  return w.numpy(), v.numpy(), be.syev_sweeps


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('kind,n', CASES)
def test_syev_stays_within_four_times_the_transcription(be, kind, n, dtype):
  a = ec.matrix(kind, n, dtype)
  t = be.from_numpy(a)
  w, v = be.syev(t)
  sweeps = be.syev_sweeps
  assert w is not t and v is not t and w.dtype == np.dtype(dtype) and v.dtype == np.dtype(dtype)
  assert tuple(w.shape) == (n,) and tuple(v.shape) == (n, n)
  assert t.numpy().tobytes() == a.tobytes()                        # the input is bit for bit what it was
  w, v = w.numpy(), v.numpy()
  yard = ec.yardstick(kind, n, dtype)
  label = 'syev %s n=%d %s' % (kind, n, np.dtype(dtype).name)
  print('%s: sweeps = %d (transcription %d, cap %d)' % (label, sweeps, yard[3], ec.MAX_SWEEPS))
  assert np.all(np.isfinite(w)) and np.all(np.isfinite(v))
  assert np.all(w[1:] >= w[:-1])                                   # ascending
  assert 0 <= sweeps <= ec.MAX_SWEEPS                              # (info == 0: syev did not raise)
  ec.check(label, a, w, v, yard)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', (37, 65))
def test_info_and_sweeps_through_the_kernel_binding(be, n, dtype):
  a = ec.matrix('pm', n, dtype)
  t, w, v, info = be.from_numpy(a), be.empty((n,), dtype), be.empty((n, n), dtype), be.from_numpy(np.array([7], np.int32))
  sweeps = kernels.syevj(t, w, v, info)
  assert int(info.numpy()[0]) == 0 and 1 <= sweeps <= ec.MAX_SWEEPS
  assert t.numpy().tobytes() == a.tobytes()
  w2, v2 = be.syev(t)
  assert w2.numpy().tobytes() == w.numpy().tobytes() and v2.numpy().tobytes() == v.numpy().tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', (40, 65))
def test_a_strided_view_gives_what_its_contiguous_copy_gives(be, n, dtype):
  a = ec.matrix('indef', n, dtype)
  frame = np.full((n + 2, n + 5), -77.0, dtype)
  frame[1:n + 1, 2:n + 2] = a
  buf = be.from_numpy(frame)
  w, v = be.syev(buf[1:n + 1, 2:n + 2])                            # lda = n + 5
  w0, v0 = be.syev(be.from_numpy(a))
  assert buf.numpy().tobytes() == frame.tobytes()
  assert w.numpy().tobytes() == w0.numpy().tobytes() and v.numpy().tobytes() == v0.numpy().tobytes()
  # V written into a view with ldv > n: the surroundings stay
  out = be.from_numpy(np.full((n + 1, n + 3), -5.0, dtype))
  wv, info = be.empty((n,), dtype), be.zeros((1,), np.int32)
  kernels.syevj(be.from_numpy(a), wv, out[1:, 3:], info)
  got = out.numpy()
  assert got[1:, 3:].tobytes() == v0.numpy().tobytes() and np.all(got[0] == -5.0) and np.all(got[:, :3] == -5.0)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', (40, 65))
def test_the_strict_upper_triangle_is_not_read(be, n, dtype):
  a = ec.matrix('indef', n, dtype)
  dirty = np.tril(a) + np.triu(np.full((n, n), np.nan, dtype), 1)
  w, v, _ = _solve(be, dirty)
  w0, v0, _ = _solve(be, a)
  assert w.tobytes() == w0.tobytes() and v.tobytes() == v0.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', (5, 64, 70))
def test_a_diagonal_matrix_needs_no_sweep(be, n, dtype):
  d = np.random.RandomState(3).permutation(n).astype(dtype) - n // 2
  d[n // 2] = d[0]                                                 # a tie: the smaller index comes first
  w, v, sweeps = _solve(be, np.diag(d))
  order = np.argsort(d, kind='stable')
  assert sweeps == 0
  assert w.tobytes() == d[order].tobytes()
  perm = np.zeros((n, n), dtype)
  perm[order, np.arange(n)] = 1
  assert v.tobytes() == perm.tobytes()


@pytest.mark.parametrize('dtype', (np.int32, np.float16), ids=lambda d: np.dtype(d).name)
def test_other_dtypes_are_refused(be, dtype):
  sq = be.from_numpy(np.eye(4).astype(dtype))
  with pytest.raises(TypeError, match='astype'):
    be.syev(sq)
  assert _hip.extras().sp_syevj(_hip.sp_dtype(dtype), None, 4, 4, None, None, 4, None, 0, None, None, None) != 0
  assert b'astype' in _hip.lib().sp_last_error()


def test_shapes_refused_and_empty_operands(be):
  with pytest.raises(ValueError):
    be.syev(be.from_numpy(np.ones((3, 4), np.float32)))
  for dtype in DTYPES:
    w, v = be.syev(D.empty((0, 0), dtype))
    assert tuple(w.shape) == (0,) and tuple(v.shape) == (0, 0) and w.dtype == np.dtype(dtype)
    w, v = be.syev(be.from_numpy(np.array([[-3.5]], dtype)))
    assert w.numpy().tolist() == [-3.5] and v.numpy().tolist() == [[1.0]] and be.syev_sweeps == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', (6, 65))
def test_a_nan_ends_at_the_sweep_cap_and_raises(be, n, dtype):
  a = ec.matrix('indef', n, dtype).copy()
  a[n // 2, 1] = np.nan
  t = be.from_numpy(a)
  with pytest.raises(np.linalg.LinAlgError, match='did not converge'):
    be.syev(t)
  assert be.syev_sweeps == ec.MAX_SWEEPS
  w, v, info = be.empty((n,), dtype), be.empty((n, n), dtype), be.zeros((1,), np.int32)
  assert kernels.syevj(t, w, v, info) == ec.MAX_SWEEPS and int(info.numpy()[0]) == 1
  # the backend is whole afterwards
  good = ec.matrix('indef', n, dtype)
  w, v, _ = _solve(be, good)
  ec.check('after the NaN, n=%d %s' % (n, np.dtype(dtype).name), good, w, v, ec.yardstick('indef', n, dtype))


def test_the_eig_header_lists_the_exports_and_the_workspace_is_sized():
  import os
  from tests.test_abi_cpu import ROOT, _declared_functions
  assert _declared_functions(os.path.join(ROOT, 'include', 'spartan_hip_eig.h')) == sorted(_hip.EXPORTS_EIG)
  x = _hip.extras()
  for dt, es, lds in ((_hip.SP_F32, 4, 64), (_hip.SP_F64, 8, 63)):
    assert x.sp_syevj_workspace_bytes(dt, 0) > 0
    assert 2 * lds * lds * es <= x.sp_syevj_workspace_bytes(dt, lds) < 4 * lds * lds * es      # A and V, once
    assert x.sp_syevj_workspace_bytes(dt, 257) >= 4 * 257 * 257 * es                             # both, twice
