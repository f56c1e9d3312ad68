"""The swaption cases on the CPU: the NumPy body of examples/_swaption.py against the literal transcription of the
reference's array program (tests/swaption_cases.oracle), the two conditions on the derived bound, the one refusing
function, and header, binding and library against each other."""
import ctypes
import os
import re

import numpy as np
import pytest

from spartan_amd import _hip, tile_checks
from spartan_amd.examples import _swaption
from tests import swaption_cases as wc

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)


def _benchmark_shapes():
  return sorted(set(wc.steps_of(ts, te) + (lamb,) for ts, te, lamb in wc.products()))


EDGE_SHAPES = ((1, 2, 0.2), (wc.MAX_K - 1, wc.MAX_K, 0.2), (1, wc.MAX_K, 0.2))


@pytest.mark.parametrize('s,k,lamb', _benchmark_shapes() + list(EDGE_SHAPES))
def test_the_float64_body_is_the_oracle_byte_for_byte(s, k, lamb):
  for n in (1, 10, 67):
    eps = wc.draws(s, n, F64)
    kept = eps.copy()
    got = _swaption.payoffs_numpy(eps, k, lamb, wc.DELTA, wc.F_0, wc.THETA)
    assert got.shape == (n,) and got.dtype == F64 and np.isfinite(got).all()
    assert got.tobytes() == wc.oracle(eps, k, lamb).tobytes(), (s, k, n)
    assert eps.tobytes() == kept.tobytes()                       # no operand is written
  assert got.any()


@pytest.mark.parametrize('dtype', (F32, F64), ids=lambda d: d.name)
def test_a_band_of_pairs_equals_the_whole(dtype):
  for s, k, lamb in ((2, 8, 0.2), (36, 40, 0.1), (1, wc.MAX_K, 0.2)):
    eps = wc.draws(s, 257, dtype)
    whole = _swaption.payoffs_numpy(eps, k, lamb, wc.DELTA, wc.F_0, wc.THETA)
    assert whole.dtype == dtype
    for lo, hi in ((0, 1), (3, 68), (100, 257), (256, 257)):
      # a column view of the wider array, and a copy of it
      for band in (eps[:, lo:hi], np.ascontiguousarray(eps[:, lo:hi])):
        assert _swaption.payoffs_numpy(band, k, lamb, wc.DELTA, wc.F_0, wc.THETA).tobytes() == whole[lo:hi].tobytes()
    assert wc.oracle(eps[:, 3:68], k, lamb).tobytes() == wc.oracle(eps, k, lamb)[3:68].tobytes()


def _all_cases():
  """(s, k, lamb, n) of every case the tests use the bound for."""
  cases = [wc.N_SHAPE[:2] + (wc.N_SHAPE[2], n) for n in wc.NS]
  cases += [(s, k, lamb, 65) for s, k, lamb in wc.SHAPES]
  cases += [wc.steps_of(ts, te) + (lamb, wc.NUM_PATHS) for ts, te, lamb in wc.products()]
  return cases


@pytest.mark.parametrize('s,k,lamb,n', _all_cases())
def test_the_bound_is_neither_loose_nor_short(s, k, lamb, n):
  """Below the cap of the case's mean payoff in both dtypes; above the error of an implementation whose exp is NumPy's
  (the float32 body against the float64 oracle; the float64 body IS the float64 oracle, and is held against a
  longdouble-free check of its own bound's size only)."""
  for dt in (F32, F64):
    eps = wc.draws(s, n, dt)
    limit = wc.bound(eps, k, lamb)
    want = wc.oracle(eps.astype(F64), k, lamb)
    mean = float(want.mean())
    assert limit.shape == (n,) and (limit > 0).all() and mean > 0
    room = wc.CAP[dt] * mean / float(limit.max())
    got = _swaption.payoffs_numpy(eps, k, lamb, wc.DELTA, wc.F_0, wc.THETA)
    used = wc.share(got, want, limit)
    print('(S, K, lamb, n) = (%d, %d, %g, %d) %s: mean payoff %.3g, bound %.3g (1 / %.0f of the cap), NumPy body at %.3g '
          'of the bound' % (s, k, lamb, n, dt.name, mean, float(limit.max()), room, used))
    assert room >= 1.0
    assert used <= 1.0
    if dt == F32:
      assert used > 0 or n < 3                                  # the float32 body does differ: the check bites


def test_the_oracle_in_float32_stays_float32_and_inside_the_bound():
  for s, k, lamb in ((2, 8, 0.2), (36, 40, 0.1)):
    eps = wc.draws(s, 65, F32)
    got = wc.oracle(eps, k, lamb)
    assert got.dtype == F32
    assert wc.share(got, wc.oracle(eps.astype(F64), k, lamb), wc.bound(eps, k, lamb)) <= 1.0
    # the float32 body and the float32 oracle: the same operations on the same NumPy
    assert got.tobytes() == _swaption.payoffs_numpy(eps, k, lamb, wc.DELTA, wc.F_0, wc.THETA).tobytes()


def test_special_draws_stay_in_their_pair():
  eps = wc.draws(4, 9, F64)
  want = _swaption.payoffs_numpy(eps, 8, 0.2, wc.DELTA, wc.F_0, wc.THETA)
  eps[2, 5] = np.nan
  got = _swaption.payoffs_numpy(eps, 8, 0.2, wc.DELTA, wc.F_0, wc.THETA)
  assert np.isnan(got).tolist() == [i == 5 for i in range(9)]
  assert np.delete(got, 5).tobytes() == np.delete(want, 5).tobytes()
  assert np.isnan(wc.oracle(eps, 8, 0.2)).tolist() == np.isnan(got).tolist()
  # lamb = 0: every exp argument is 0, f stays f0
  flat = _swaption.payoffs_numpy(wc.draws(4, 9, F64), 8, 0.0, wc.DELTA, wc.F_0, wc.THETA)
  assert len(set(flat.tolist())) == 1 and flat.tobytes() == wc.oracle(wc.draws(4, 9, F64), 8, 0.0).tobytes()


def test_every_refusal_of_the_check():
  ok = dict(dtype=F32, shape=(2, 9), maturities=8, lamb=0.2, delta=0.5, f0=0.06, theta=0.06)
  assert tile_checks.check_lmm_swaption(**ok) == (F32, 9, 2, 8, 0.2, 0.5, 0.06, 0.06)
  assert tile_checks.check_lmm_swaption(steps=2, **ok)[2] == 2
  assert tile_checks.check_lmm_swaption(**dict(ok, shape=(2, 0)))[1] == 0
  assert tile_checks.check_lmm_swaption(**dict(ok, shape=(wc.MAX_K - 1, 3), maturities=wc.MAX_K))[2:4] == (wc.MAX_K - 1, wc.MAX_K)
  cases = [
      (TypeError, 'astype first', dict(dtype=np.int32)),
      (TypeError, 'astype first', dict(dtype=np.float16)),
      (TypeError, 'astype first', dict(dtype=np.complex128)),
      (ValueError, r'draws of shape \(steps, n\)', dict(shape=(9,))),
      (ValueError, r'draws of shape \(steps, n\)', dict(shape=(2, 9, 1))),
      (ValueError, r'draws of shape \(3, n\)', dict(steps=3)),
      (ValueError, 'steps = 0 and maturities = 8', dict(shape=(0, 9))),
      (ValueError, 'steps = 2 and maturities = 2', dict(maturities=2)),
      (ValueError, 'steps = 2 and maturities = 1', dict(maturities=1)),
      (ValueError, 'maturities = %d' % (wc.MAX_K + 1), dict(maturities=wc.MAX_K + 1)),
      (ValueError, 'lamb = nan must be finite', dict(lamb=float('nan'))),
      (ValueError, 'lamb = inf must be finite', dict(lamb=float('inf'))),
      (ValueError, 'f0 = 1e\\+39 must be finite in float32', dict(f0=1e39)),
      (ValueError, 'theta = -inf must be finite', dict(theta=float('-inf'))),
      (ValueError, 'delta = nan must be finite', dict(delta=float('nan'))),
      (ValueError, 'delta = 0.0 must be > 0', dict(delta=0.0)),
      (ValueError, 'delta = -0.5 must be > 0', dict(delta=-0.5)),
      (ValueError, 'delta = 1e-50 must be > 0 in float32', dict(delta=1e-50)),
  ]
  for exc, match, change in cases:
    with pytest.raises(exc, match=match):
      tile_checks.check_lmm_swaption(**dict(ok, **change))
  assert tile_checks.check_lmm_swaption(**dict(ok, dtype=F64, f0=1e39, delta=1e-50))[0] == F64
  # the NumPy path of the dispatcher refuses through the same function
  import spartan_amd as sp
  from oracle.np_backend import NumpyBackend
  sp.initialize(backend=NumpyBackend(), num_workers=1)
  try:
    with pytest.raises(TypeError, match='astype first'):
      _swaption.lmm_swaption(np.zeros((2, 3), np.int64), 8, 0.2)
    with pytest.raises(ValueError, match='steps = 2 and maturities = 2'):
      _swaption.lmm_swaption(np.zeros((2, 3)), 2, 0.2)
    got = _swaption.lmm_swaption(wc.draws(2, 5, F64), 8, 0.2)
    assert np.asarray(got).tobytes() == wc.oracle(wc.draws(2, 5, F64), 8, 0.2).tobytes()
  finally:
    sp.shutdown()


def test_the_lmm_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  header = os.path.join(ROOT, 'include', 'spartan_hip_lmm.h')
  names = _declared_functions(header)
  assert names == sorted(_hip.EXPORTS_LMM) == ['sp_lmm_swaption']
  others = (set(_hip.EXPORTS) | set(_hip.EXPORTS_EXTRAS) | set(_hip.EXPORTS_EIG) | set(_hip.EXPORTS_KNN)
            | set(_hip.EXPORTS_GRAPH) | set(_hip.EXPORTS_ALS) | set(_hip.EXPORTS_FUZZY) | set(_hip.EXPORTS_LDA)
            | set(_hip.EXPORTS_SPECTRAL) | set(_hip.EXPORTS_NB) | set(_hip.EXPORTS_NBODY) | set(_hip.EXPORTS_CF)
            | set(_hip.EXPORTS_SVM) | set(_hip.EXPORTS_MF))
  for h in (EXTRAS_HEADER,) + tuple(os.path.join(ROOT, 'include', 'spartan_hip_%s.h' % s) for s in
                                    ('eig', 'knn', 'graph', 'als', 'fuzzy', 'lda', 'spectral', 'nb', 'nbody', 'cf', 'svm', 'mf')):
    others |= set(_declared_functions(h))
  assert not set(names) & others
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  text = open(header).read()
  assert int(re.search(r'#define SP_LMM_MAX_K (\d+)', text).group(1)) == _hip.SP_LMM_MAX_K >= 128
  # 64 pairs of K doubles are the workgroup's LDS: within the 64 KiB a workgroup may ask for
  assert _hip.SP_LMM_MAX_K * 64 * 8 <= 65536
  from spartan_amd.backend_hip import HipBackend
  from spartan_amd.backend_hip_lmm import LmmTileBodies
  assert issubclass(HipBackend, LmmTileBodies)
  assert [m for m in vars(LmmTileBodies) if not m.startswith('_')] == ['lmm_swaption']
