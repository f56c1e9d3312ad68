"""sp_svm_dca (csrc/svm.hip) through HipBackend.svm_dca and kernels.svm_dca against the stated order of
tests/svm_cases.restated, byte for byte, alpha and w alike, in both dtypes.

Shapes, for the kernel that was built (include/spartan_hip_svm.h): m = 0, 1, 2, 63, 64, 65 and 200 rows sit on both
sides of the ring's batches (8, 4, 2 or 1 rows, two in flight) and of a wave's 64 lanes; d = 1, 3, 63, 64, 65, 130 and
1000 take the register buckets of 1, 2, 4 and 16 values per lane, 300 and 520 the buckets of 8 and 16 at a padded width,
2000 the LDS bucket of 32 and 4096 (with 5 rows) that of 64 -- in float64 the one that reads a row where it is used;
chains = 1, 2, 3, 7, m and m + 3 leave workgroups partly filled and chains without rows.  Nothing is larger."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, kernels, tile_checks
from tests import svm_cases as sc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
dtype_ids = dict(ids=lambda d: np.dtype(d).name)


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _run(be, x, y, alpha, w0, s, chains, want_w=True):
  out = be.svm_dca(*(be.from_numpy(np.ascontiguousarray(v)) for v in (x, y, alpha, w0)), s, chains=chains, want_w=want_w)
  return tuple(t.numpy() for t in out) if want_w else out.numpy()


def _check(be, m, d, chains, dtype, seed=0):
  x, y, alpha, w0, s = sc.case(m, d, dtype, seed)
  before = be.launches
  got_a, got_w = _run(be, x, y, alpha, w0, s, chains)
  assert be.launches - before == 1                                # one kernel, whatever the shape
  want_a, want_w = sc.restated(x, y, alpha, w0, s, chains)
  assert got_a.shape == (m, 1) and got_w.shape == (chains, d) and got_a.dtype == got_w.dtype == np.dtype(dtype)
  assert got_a.reshape(m).tobytes() == want_a.tobytes(), (m, d, chains)
  assert got_w.tobytes() == want_w.tobytes(), (m, d, chains)
  return x, y, alpha, w0, s, got_a, got_w


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('m', sc.MS)
def test_rows_and_chains(be, m, dtype):
  for chains in sorted(set((1, 2, 3, 7, max(m, 1), m + 3))):
    _check(be, m, 3, chains, dtype)
  if m in (65, 200):
    _check(be, m, 64, 7, dtype)
    _check(be, m, 130, 2, dtype)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('d', sc.DS + (300, 520, 2000))
def test_features(be, d, dtype):
  m = 65 if d <= 130 else 19
  for chains in (1, 3):
    x, y, alpha, w0, s, got_a, got_w = _check(be, m, d, chains, dtype)
  assert _run(be, x, y, alpha, w0, s, 3)[0].tobytes() == got_a.tobytes()       # a repeated call: the same bytes
  # without w: the same alpha
  assert _run(be, x, y, alpha, w0, s, 3, want_w=False).tobytes() == got_a.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_the_widest_row(be, dtype):
  m, d = sc.BIG_D
  _check(be, m, d, 1, dtype)
  _check(be, m, d, 2, dtype)
  _check(be, m, d, m + 3, dtype)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_chains_are_calls_on_the_bands(be, dtype):
  m, d = 65, 7
  x, y, alpha, w0, s = sc.case(m, d, dtype)
  whole_a, whole_w = _run(be, x, y, alpha, w0, s, 4)
  for c, (lo, hi) in enumerate(sc.chain_rows(m, 4)):
    a, w = _run(be, x[lo:hi], y[lo:hi], alpha[lo:hi], w0, s, 1)
    assert whole_a[lo:hi].tobytes() == a.tobytes() and whole_w[c].tobytes() == w[0].tobytes()


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_strides_views_and_alpha_in_place(be, dtype):
  dt = np.dtype(dtype)
  m, d = 65, 7
  x, y, alpha, w0, s = sc.case(m, d, dt)
  want_a, want_w = sc.restated(x, y, alpha, w0, s, 3)
  # ldx = d + 3: a row view of a wider array, taken as it is (no copy is counted or made)
  wide = np.full((m, d + 3), 7.0, dt)
  wide[:, :d] = x
  wide_t = be.from_numpy(wide)
  view = wide_t[:, :d]
  assert view.stride(0) == d + 3 and be._unit_rows(view) is view
  ops = [be.from_numpy(v) for v in (y.reshape(m, 1), alpha, w0.reshape(d, 1))]
  before = be.launches
  a, w = be.svm_dca(view, ops[0], ops[1], ops[2], s, chains=3, want_w=True)
  assert be.launches - before == 1
  assert a.numpy().reshape(m).tobytes() == want_a.tobytes() and w.numpy().tobytes() == want_w.tobytes()
  assert wide_t.numpy().tobytes() == wide.tobytes()                      # no operand is written
  # a column of a wider array for y and alpha, a transposed x: copied first, the same bytes, still one launch
  ya = np.zeros((m, 2), dt)
  ya[:, 0], ya[:, 1] = y, alpha
  ya_t = be.from_numpy(ya)
  xt = be.from_numpy(np.ascontiguousarray(x.T))
  before = be.launches
  a = be.svm_dca(xt.t(), ya_t[:, 0], ya_t[:, 1:2], ops[2], s, chains=3)
  assert be.launches - before == 1 and a.numpy().reshape(m).tobytes() == want_a.tobytes()
  # the launcher with alpha_out = alpha: in place
  xd, yd, ad, wd = (be.from_numpy(v) for v in (x, y, alpha, w0))
  w_out = be.empty((3, d), dt)
  kernels.svm_dca(xd, yd, ad, wd, s, 3, ad, w_out=w_out)
  assert ad.numpy().tobytes() == want_a.tobytes() and w_out.numpy().tobytes() == want_w.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_special_rows(be, dtype):
  """The rows of tests/svm_cases.special_case: the stated order's values, a NaN where it has one (svm_cases.same)."""
  x, y, alpha, w0, s = sc.special_case(dtype)
  got_a, got_w = _run(be, x, y, alpha, w0, s, 1)
  want_a, want_w = sc.restated(x, y, alpha, w0, s, 1)
  assert sc.same(got_a.reshape(-1), want_a) and sc.same(got_w, want_w)
  assert np.isnan(got_w[0]).tolist() == np.isnan(x[sc.SPECIAL_ROWS['NaN in x']]).tolist()
  # ... and up to the NaN row by bytes alone
  i = sc.SPECIAL_ROWS['NaN in x']
  got_a, got_w = _run(be, x[:i], y[:i], alpha[:i], w0, s, 1)
  want_a, want_w = sc.restated(x[:i], y[:i], alpha[:i], w0, s, 1)
  assert got_a.reshape(-1).tobytes() == want_a.tobytes() and got_w.tobytes() == want_w.tobytes()


def test_refusals_launch_nothing(be):
  f32 = np.dtype(np.float32)
  x, y, alpha, w0, s = sc.case(9, 3, f32)
  dev = lambda v: be.from_numpy(np.ascontiguousarray(v))   # noqa: E731
  xd, yd, ad, wd = (dev(v) for v in (x, y, alpha, w0))
  out = be.empty((9, 1), f32)
  cases = [
      (TypeError, 'astype', dict(x=dev(x.astype(np.int32)))),
      (TypeError, 'astype', dict(y=dev(y.astype(np.float64)))),
      (ValueError, r'\(m, d\)', dict(x=dev(x.reshape(-1)))),
      (ValueError, 'y of shape', dict(y=dev(y[:8]))),
      (ValueError, 'alpha of shape', dict(alpha=dev(alpha.reshape(3, 3)))),
      (ValueError, 'w0 of shape', dict(w0=dev(w0[:2]))),
      (ValueError, 'chains', dict(chains=0)),
      (ValueError, 'scaled_lambda', dict(s=0.0)),
      (ValueError, 'scaled_lambda', dict(s=float('nan'))),
      (ValueError, 'd = %d' % (_hip.SP_SVM_MAX_D + 1),
       dict(x=dev(np.zeros((9, _hip.SP_SVM_MAX_D + 1), f32)), w0=dev(np.zeros(_hip.SP_SVM_MAX_D + 1, f32)))),
  ]
  for exc, match, change in cases:
    kw = dict(x=xd, y=yd, alpha=ad, w0=wd, s=s, chains=1)
    kw.update(change)
    shapes = [tuple(kw[k].shape) for k in ('x', 'y', 'alpha', 'w0')]
    with pytest.raises(exc, match=match):                     # the check itself, the backend and the launcher alike
      tile_checks.check_svm_dca([be.dtype_of(kw[k]) for k in ('x', 'y', 'alpha', 'w0')], shapes, kw['s'], kw['chains'])
    before = be.launches
    with pytest.raises(exc, match=match):
      be.svm_dca(kw['x'], kw['y'], kw['alpha'], kw['w0'], kw['s'], chains=kw['chains'])
    with pytest.raises(exc, match=match):
      kernels.svm_dca(kw['x'], kw['y'], kw['alpha'], kw['w0'], kw['s'], kw['chains'], out)
    assert be.launches == before
  # targets that do not fit, and the library's own refusals (nothing is launched: the operands stay as they are)
  with pytest.raises(ValueError, match='targets'):
    kernels.svm_dca(xd, yd, ad, wd, s, 2, out, w_out=be.empty((3, 3), f32))
  with pytest.raises(TypeError, match='astype'):
    kernels.svm_dca(xd, yd, ad, wd, s, 1, be.empty((9, 1), np.float64))
  lib = _hip.extras()
  p = lambda t: t.data_ptr()   # noqa: E731
  assert lib.sp_svm_dca(_hip.SP_F32, p(xd), 2, 9, 3, p(yd), p(ad), p(wd), s, 1, p(out), None, None) != 0     # ldx < d
  assert lib.sp_svm_dca(_hip.SP_F32, p(xd), 3, 9, 3, p(yd), p(ad), None, s, 1, p(out), None, None) != 0      # NULL w0
  assert lib.sp_svm_dca(_hip.SP_F32, p(xd), 3, 9, 3, p(yd), p(ad), p(wd), s, 0, p(out), None, None) != 0     # chains
  # m = 0: nothing to write without w, one launch (w0 for every chain) with it
  before = be.launches
  a = be.svm_dca(xd[:0], yd[:0], ad[:0], wd, s, chains=2)
  assert a.shape == (0, 1) and be.launches == before
  a, w = be.svm_dca(xd[:0], yd[:0], ad[:0], wd, s, chains=2, want_w=True)
  assert be.launches == before + 1 and w.numpy().tobytes() == np.stack([w0, w0]).tobytes()
