"""sp_lmm_swaption (csrc/lmm.hip) through HipBackend.lmm_swaption and kernels.lmm_swaption against the literal NumPy
transcription of the reference's array program (tests/swaption_cases.oracle) in the same dtype, inside the derived bound
of tests/swaption_cases.bound; by bytes wherever exp is out of the way.

Shapes, for the kernel that was built (include/spartan_hip_lmm.h: a workgroup is one wave of 64 pairs): n = 1, 2, 63, 64,
65, 257 and 600 at (S, K, lamb) = (2, 8, 0.2) sit on both sides of a workgroup and leave the last one partly filled;
(S, K) = (1, 2), (7, 8), (1, 40), (36, 40), (20, 40), (1, SP_LMM_MAX_K) and (SP_LMM_MAX_K - 1, SP_LMM_MAX_K) at n = 65
take the k loop's unrolled body and its remainder at every length and the whole LDS.  Nothing is larger.  The driver on
the device: the `hip` legs of tests/test_swaption_example.py."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, kernels, tile_checks
from spartan_amd.examples import _swaption
from tests import swaption_cases as wc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
dtype_ids = dict(ids=lambda d: np.dtype(d).name)


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _run(be, eps, k, lamb, **kw):
  return be.lmm_swaption(be.from_numpy(np.ascontiguousarray(eps)), k, lamb, **kw).numpy()


def _check(be, s, k, lamb, n, dtype, eps=None, theta=wc.THETA):
  dt = np.dtype(dtype)
  eps = wc.draws(s, n, dt) if eps is None else eps
  before = be.launches
  got = _run(be, eps, k, lamb, theta=theta)
  assert be.launches - before == 1                                  # one kernel, whatever the shape
  assert got.shape == (n,) and got.dtype == dt
  want, limit = wc.oracle(eps, k, lamb, theta=theta), wc.bound(eps, k, lamb, theta=theta)
  used = wc.share(got, want, limit)
  print('(S, K, lamb, n) = (%d, %d, %g, %d) %s: the kernel is at %.3g of the bound (largest bound %.3g, mean payoff %.3g)'
        % (s, k, lamb, n, dt.name, used, float(limit.max()), float(want.mean())))
  assert used <= 1.0, (s, k, n, dt)
  return eps, got


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('n', wc.NS)
def test_pairs_inside_the_bound(be, n, dtype):
  s, k, lamb = wc.N_SHAPE
  _check(be, s, k, lamb, n, dtype)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('s,k,lamb', wc.SHAPES)
def test_shapes_inside_the_bound(be, s, k, lamb, dtype):
  _check(be, s, k, lamb, 65, dtype)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('s,k', ((2, 8), (36, 40)))
def test_without_exp_the_bytes_are_numpys(be, s, k, dtype):
  """lamb = 0: every exp argument is exactly 0 and f stays f0 -- the bond chain, the discount product, the final
  subtraction and the IEEE divisions with no exp in the way."""
  eps = wc.draws(s, 65, dtype)
  got = _run(be, eps, k, 0.0)
  want = _swaption.payoffs_numpy(eps, k, 0.0, wc.DELTA, wc.F_0, wc.THETA)
  assert got.tobytes() == want.tobytes()                  # (at the money, theta = f0: zeros, or a rounding's worth)
  # ... and in the money, with other parameters, whose constants are formed on the host
  got = _run(be, eps, k, 0.0, delta=0.3, f0=0.041, theta=0.013)
  assert got.tobytes() == _swaption.payoffs_numpy(eps, k, 0.0, 0.3, 0.041, 0.013).tobytes() and got.any()


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_an_antithetic_pair_on_one_path(be, dtype):
  """All draws 0: both signs follow the same path, every output is the same value -- 0 at the reference's strike, which
  is the start rate; a payoff at half of it."""
  eps = np.zeros((4, 65), dtype)
  _, got = _check(be, 4, 8, 0.2, 65, dtype, eps=eps)
  assert len(set(got.tolist())) == 1
  _, got = _check(be, 4, 8, 0.2, 65, dtype, eps=eps, theta=0.03)
  assert len(set(got.tolist())) == 1 and got[0] > 0


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_a_band_alone_a_repeat_and_a_strided_operand(be, dtype):
  dt = np.dtype(dtype)
  s, k, lamb, n = 6, 10, 0.2, 257
  eps = wc.draws(s, n, dt)
  wide = be.from_numpy(eps)
  whole = be.lmm_swaption(wide, k, lamb).numpy()
  assert be.lmm_swaption(wide, k, lamb).numpy().tobytes() == whole.tobytes()        # a repeated call: the same bytes
  for a, b in ((0, 1), (3, 68), (64, 128), (100, 257), (256, 257)):
    view = wide[:, a:b]
    assert (b - a == 1 or view.stride(0) == n) and be._unit_rows(view) is view        # ld_eps > n, taken as it is
    before = be.launches
    got = be.lmm_swaption(view, k, lamb)
    assert be.launches - before == 1
    assert got.numpy().tobytes() == whole[a:b].tobytes(), (a, b)
  assert wide.numpy().tobytes() == eps.tobytes()                                      # the draws are not written
  # a transposed operand is copied first: the same bytes, still one launch
  t = be.from_numpy(np.ascontiguousarray(eps.T))
  before = be.launches
  got = be.lmm_swaption(t.t(), k, lamb)
  assert be.launches - before == 1 and got.numpy().tobytes() == whole.tobytes()
  # the launcher on a band of a wider array, into a target of its own
  out = be.empty((65,), dt)
  assert kernels.lmm_swaption(wide[:, 3:68], k, lamb, wc.DELTA, wc.F_0, wc.THETA, out) is out
  assert out.numpy().tobytes() == whole[3:68].tobytes()
  # a host array goes to the device by itself
  assert be.lmm_swaption(eps, k, lamb).numpy().tobytes() == whole.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_a_nan_stays_in_its_pair(be, dtype):
  s, k, lamb, n = 4, 8, 0.2, 130
  eps = wc.draws(s, n, dtype)
  clean = _run(be, eps, k, lamb)
  for row, col in ((0, 0), (2, 70), (3, 129)):
    bad = eps.copy()
    bad[row, col] = np.nan
    got = _run(be, bad, k, lamb)
    assert np.isnan(got).tolist() == [i == col for i in range(n)]
    assert np.delete(got, col).tobytes() == np.delete(clean, col).tobytes()


def test_no_pairs_no_launch(be):
  for dt in DTYPES:
    before = be.launches
    out = be.lmm_swaption(be.from_numpy(np.zeros((2, 4), dt))[:, :0], 8, 0.2)
    assert out.shape == (0,) and be.dtype_of(out) == np.dtype(dt) and be.launches == before
  lib = _hip.extras()
  assert lib.sp_lmm_swaption(_hip.SP_F32, None, 0, 0, 2, 8, 0.2, 0.5, 0.06, 0.06, None, None) == 0


def test_refusals_launch_nothing(be):
  f32 = np.dtype(np.float32)
  eps = wc.draws(2, 9, f32)
  dev = lambda v: be.from_numpy(np.ascontiguousarray(v))   # noqa: E731
  ed = dev(eps)
  out = be.empty((9,), f32)
  cases = [
      (TypeError, 'astype first', dict(eps=dev(eps.astype(np.int32)))),
      (ValueError, r'draws of shape \(steps, n\)', dict(eps=dev(eps.reshape(-1)))),
      (ValueError, 'steps = 2 and maturities = 2', dict(k=2)),
      (ValueError, 'maturities = %d' % (wc.MAX_K + 1), dict(k=wc.MAX_K + 1)),
      (ValueError, 'lamb = nan', dict(lamb=float('nan'))),
      (ValueError, 'f0 = inf', dict(f0=float('inf'))),
      (ValueError, 'theta = 1e\\+39 must be finite in float32', dict(theta=1e39)),
      (ValueError, 'delta = 0.0 must be > 0', dict(delta=0.0)),
      (ValueError, 'delta = -0.5 must be > 0', dict(delta=-0.5)),
  ]
  for exc, match, change in cases:
    kw = dict(eps=ed, k=8, lamb=0.2, delta=wc.DELTA, f0=wc.F_0, theta=wc.THETA)
    kw.update(change)
    with pytest.raises(exc, match=match):                     # the check itself, the backend and the launcher alike
      tile_checks.check_lmm_swaption(be.dtype_of(kw['eps']), tuple(kw['eps'].shape), kw['k'], kw['lamb'], kw['delta'],
                                     kw['f0'], kw['theta'])
    before = be.launches
    with pytest.raises(exc, match=match):
      be.lmm_swaption(kw['eps'], kw['k'], kw['lamb'], delta=kw['delta'], f0=kw['f0'], theta=kw['theta'])
    with pytest.raises(exc, match=match):
      kernels.lmm_swaption(kw['eps'], kw['k'], kw['lamb'], kw['delta'], kw['f0'], kw['theta'], out)
    assert be.launches == before
  # targets that do not fit
  with pytest.raises(ValueError, match='target of shape'):
    kernels.lmm_swaption(ed, 8, 0.2, wc.DELTA, wc.F_0, wc.THETA, be.empty((8,), f32))
  with pytest.raises(TypeError, match='astype'):
    kernels.lmm_swaption(ed, 8, 0.2, wc.DELTA, wc.F_0, wc.THETA, be.empty((9,), np.float64))
  # the library's own refusals: an error code, and the target keeps its bytes (nothing was launched)
  marks = np.full(9, 7.0, f32)
  out = dev(marks)
  lib = _hip.extras()
  p = lambda t: t.data_ptr()   # noqa: E731
  ok = dict(dtype=_hip.SP_F32, eps=p(ed), ld=9, n=9, s=2, k=8, lamb=0.2, delta=0.5, f0=0.06, theta=0.06, out=p(out))
  bad = [dict(dtype=99), dict(n=-1), dict(ld=8), dict(s=0), dict(s=8), dict(s=9),
         dict(k=wc.MAX_K + 1), dict(s=wc.MAX_K, k=wc.MAX_K), dict(lamb=float('nan')), dict(lamb=float('inf')),
         dict(delta=float('nan')), dict(delta=0.0), dict(delta=-0.5), dict(delta=1e-50), dict(f0=float('inf')),
         dict(f0=1e39), dict(theta=float('-inf')), dict(eps=None), dict(out=None)]
  for change in bad:
    a = dict(ok, **change)
    rc = lib.sp_lmm_swaption(a['dtype'], a['eps'], a['ld'], a['n'], a['s'], a['k'], a['lamb'], a['delta'], a['f0'],
                             a['theta'], a['out'], None)
    assert rc != 0, change
  assert out.numpy().tobytes() == marks.tobytes()
