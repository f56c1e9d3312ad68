"""examples/swaption: the swaption driver on the injected NumPy backend at 1 and 4 workers, where the tile body is the
NumPy recurrence beside the driver (examples/_swaption.py).  GPU leg (marked): the golden runs on the HIP backend
(sp_lmm_swaption) at 1 and 4 logical workers.

Input and reference: tests/golden/swaption_w4.npz, recorded by tests/golden/make_golden_swaption.py: the 16 products of
the reference's benchmark with 10 paths, each with its draws and its [mean, std].  whole_run is 0 in the recorded file:
the reference's simulate does not evaluate at this revision (the script's docstring says what stops it), and the
results are those of the literal NumPy float64 transcription of its array program (tests/swaption_cases.oracle) on the
recorded draws.

Tolerances: per pair the NumPy body is that program bit for bit, so only the order of the two 10-term reductions
differs -- the mean to 1e-12 relative; std's mean(a^2) - mean(a)^2 amplifies that by about (mean / std)^2, below 100
for these products -- the std to 1e-9 relative.  On the device both are widened by the kernel's derived bound
(tests/swaption_cases.bound): the mean by the mean of the pairs' bounds, the std -- which moves by at most the largest
change of an element, std(a + d) <= std(a) + std(d) -- by the largest, divided by sqrt(num_paths)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples import _swaption, swaption
from tests import swaption_cases as wc

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
BACKENDS = ('numpy', pytest.param('hip', marks=pytest.mark.gpu))


def start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _numbers(result):
  return np.asarray([[float(np.asarray(me.glom())), float(np.asarray(st.glom()))] for me, st in result])


def golden_run(backend, workers, method, dtype, device_bound=False):
  """The 16 products on the golden's draws against its results; returns the [mean, std] pairs as host arrays."""
  dt = np.dtype(dtype)
  g = wc.golden()
  assert g['whole_run'] in (0, 1) and len(g['eps_all']) == 16 == len(wc.products())
  assert g['products'].tolist() == [list(map(float, p)) for p in wc.products()]
  start(backend, workers)
  try:
    asked, body = [], _swaption.lmm_swaption

    def watched(eps, maturities, lamb, **kw):
      asked.append((tuple(eps.shape), maturities, lamb))
      return body(eps, maturities, lamb, **kw)
    _swaption.lmm_swaption = watched
    try:
      result = swaption.simulate(wc.TS_ALL, wc.TE_ALL, wc.LAMB_ALL, wc.NUM_PATHS, method=method, dtype=dt,
                                 eps_all=g['eps_all'])
    finally:
      _swaption.lmm_swaption = body
    if method == 'fused':
      # one tile body per band and product, over column bands of divup(num_paths, workers)
      band = -(-wc.NUM_PATHS // workers)
      widths = [min(band, wc.NUM_PATHS - lo) for lo in range(0, wc.NUM_PATHS, band)]
      want = [((wc.steps_of(ts, te)[0], w), wc.steps_of(ts, te)[1], lamb) for ts, te, lamb in wc.products() for w in widths]
      assert sorted(asked) == sorted(want)
    else:
      assert not asked
    got = _numbers(result)
    assert got.shape == (16, 2)
    for i, ((ts, te, lamb), eps) in enumerate(zip(wc.products(), g['eps_all'])):
      mean, std = g['results'][i]
      tol_mean, tol_std = 1e-12 * mean, 1e-9 * std
      if device_bound or dt == F32:
        limit = wc.bound(eps.astype(dt), wc.steps_of(ts, te)[1], lamb)
        tol_mean += float(limit.mean()) * 10000
        tol_std += float(limit.max()) / np.sqrt(wc.NUM_PATHS) * 10000
      if dt == F32:
        # the float32 draws are other draws: the golden's float64 results are replaced by the float64 oracle on them
        v = wc.oracle(eps.astype(F32).astype(F64), wc.steps_of(ts, te)[1], lamb)
        mean, std = v.mean() * 10000, v.std() / np.sqrt(wc.NUM_PATHS) * 10000
        tol_mean += 12 * wc.U[F32] * mean        # the float32 sum of 10 terms in any order (9 u), / 10 and * 10000
      print('%s %s at %d workers, product %d (%g, %g, %g): mean %.12g (golden %.12g, %.3g of the tolerance), std %.12g '
            '(golden %.12g, %.3g of the tolerance)' % (backend, method, workers, i, ts, te, lamb, got[i, 0], mean,
                                                       abs(got[i, 0] - mean) / tol_mean, got[i, 1], std,
                                                       abs(got[i, 1] - std) / tol_std))
      assert abs(got[i, 0] - mean) <= tol_mean, (i, got[i, 0], mean)
      assert abs(got[i, 1] - std) <= tol_std, (i, got[i, 1], std)
    return [[np.asarray(v.glom()) for v in pair] for pair in result]
  finally:
    sp.shutdown()


@pytest.mark.parametrize('method', swaption.METHODS)
@pytest.mark.parametrize('workers', (1, 4))
@pytest.mark.parametrize('backend', BACKENDS)
def test_the_golden_run(backend, workers, method):
  """whole_run is 0 in the recorded file (module docstring): the golden's results are the transcription's."""
  result = golden_run(backend, workers, method, F64, device_bound=backend == 'hip')
  assert all(v.dtype == F64 and v.shape == () for pair in result for v in pair)


@pytest.mark.parametrize('workers', (1, 4))
@pytest.mark.parametrize('backend', BACKENDS)
def test_float32_stays_float32_up_to_the_cast_of_std(backend, workers):
  result = golden_run(backend, workers, 'fused', F32, device_bound=backend == 'hip')
  for me, st in result:
    assert me.dtype == F32 and st.dtype == F64
  # the payoffs themselves are float32 tiles
  start(backend, workers)
  try:
    eps = swaption._draws(wc.golden()['eps_all'][0], 2, wc.NUM_PATHS, 3, F32)
    v = swaption._fused(eps, 2, 8, wc.NUM_PATHS, 3, 0.2, F32, wc.DELTA, wc.F_0, wc.THETA)
    assert v.dtype == F32 and np.asarray(v.glom()).dtype == F32 and v.shape == (wc.NUM_PATHS,)
  finally:
    sp.shutdown()


def test_dates_and_other_refusals():
  start('numpy', 2)
  try:
    for ts, te in ((1.25, 4), (1, 4.1), (0.3, 0.9)):
      with pytest.raises(ValueError, match='whole multiple of delta'):
        swaption.simulate([[ts]], [te], [0.2], 10)
    for ts, te in ((0, 4), (-1, 4), (4, 4), (5, 4), (1, float('inf')), (float('nan'), 4)):
      with pytest.raises(ValueError, match='0 < ts < te'):
        swaption.simulate([[ts]], [te], [0.2], 10)
    # on another grid the same dates are fine, and (0.5, 1) is the smallest product of the reference's grid
    assert len(swaption.simulate([[1.25]], [4], [0.2], 10, delta=0.25)) == 1
    assert len(swaption.simulate([[0.5]], [1], [0.2], 10)) == 1
    with pytest.raises(ValueError, match='maturities = %d' % (wc.MAX_K + 1)):
      swaption.simulate([[1]], [(wc.MAX_K + 1) * 0.5], [0.2], 10)
    with pytest.raises(ValueError, match='unknown method'):
      swaption.simulate([[1]], [4], [0.2], 10, method='plane')
    with pytest.raises(ValueError, match='num_paths = 0'):
      swaption.simulate([[1]], [4], [0.2], 0)
    with pytest.raises(TypeError, match='float32 float64'):
      swaption.simulate([[1]], [4], [0.2], 10, dtype=np.float16)
    with pytest.raises(ValueError, match='lamb = nan'):
      swaption.simulate([[1]], [4], [float('nan')], 10)
    with pytest.raises(ValueError, match='delta = 0.0'):
      swaption.simulate([[1]], [4], [0.2], 10, delta=0.0)
    with pytest.raises(ValueError, match='eps_all holds 1 arrays for 2 products'):
      swaption.simulate([[1, 2]], [4], [0.2], 10, eps_all=[np.zeros((2, 10))])
    with pytest.raises(ValueError, match=r'draws of shape \(3, 10\)'):
      swaption.simulate([[1]], [4], [0.2], 10, eps_all=[np.zeros((3, 10))])
    with pytest.raises(TypeError, match='real numbers'):
      swaption.simulate([[1]], [4], [0.2], 10, eps_all=[np.zeros((2, 10), np.complex128)])
    # draws as a distributed array, of another tiling and dtype: the bytes of the NumPy array's run
    eps = wc.draws(2, 10, F64)
    a = _numbers(swaption.simulate([[1]], [4], [0.2], 10, eps_all=[eps]))
    b = _numbers(swaption.simulate([[1]], [4], [0.2], 10, eps_all=[sp.from_numpy(eps, tile_hint=(1, 10)).evaluate()]))
    assert a.tobytes() == b.tobytes()
    assert (swaption.DELTA, swaption.F_0, swaption.THETA) == (0.5, 0.06, 0.06)
  finally:
    sp.shutdown()


@pytest.mark.parametrize('workers', (1, 4))
def test_its_own_draws(workers):
  """Two runs after the same seed agree; (1, 4, 0.2) at 4096 paths lies within 6 of its own reported standard errors of
  the oracle's value at the same size under a fixed NumPy seed (both estimates carry that error, hence 6 and not 3)."""
  paths = 4096
  start('numpy', workers)
  try:
    runs = []
    for _ in range(2):
      sp.set_random_seed(7)
      runs.append(_numbers(swaption.simulate([[1]], [4], [0.2], paths)))
    assert runs[0].tobytes() == runs[1].tobytes()
    mean, err = runs[0][0]
    v = wc.oracle(np.random.RandomState(7).randn(2, paths), 8, 0.2)
    want, want_err = v.mean() * 10000, v.std() / np.sqrt(paths) * 10000
    print('(1, 4, 0.2) at %d paths: %.3f +- %.3f bp; the oracle on NumPy draws: %.3f +- %.3f bp' % (paths, mean, err, want, want_err))
    assert 0.5 * want_err < err < 2 * want_err
    assert abs(mean - want) <= 6 * err
  finally:
    sp.shutdown()
