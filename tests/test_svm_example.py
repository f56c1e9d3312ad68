"""examples/disdca_svm: the linear SVM driver.  CPU leg: the host framework on the injected NumPy backend at 1 and 4
workers, where the tile body is the NumPy restatement beside the driver (examples/_svm.py).  GPU leg (marked): the same
checks on the HIP backend (sp_svm_dca) at 1 and 4 logical workers.

Input and reference: tests/golden/disdca_svm_w4.npz, recorded by tests/golden/make_golden_svm.py from the reference's
own fit at 4 workers (148 x 7, float64, T = 3, la = 0.1).  Accuracy: the rule of tests/svm_cases.py -- alpha after
iterations 1 and 3 and w after 3 within 8 e_ref of the longdouble yardstick (times 2^29 in float32); every ratio is
printed before it is asserted."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples import _svm, disdca_svm as svm
from tests import svm_cases as sc

BACKENDS = ('numpy', pytest.param('hip', marks=pytest.mark.gpu))
DTYPES = (np.float32, np.float64)


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _fit(x, y, iters, **kw):
  w, alpha = svm.fit_state(x, y, T=iters, la=sc.LA, **kw)
  return np.asarray(w.glom()), np.asarray(alpha.glom())


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('workers', (1, 4))
@pytest.mark.parametrize('backend', BACKENDS)
def test_the_golden_run(backend, workers, dtype):
  """4 workers x 1 chain, or 1 worker x 4 chains: the reference's four tiles either way."""
  dt = np.dtype(dtype)
  x, y = sc.golden_input()
  _start(backend, workers)
  try:
    asked, body = [], _svm.svm_dca

    def watched(xt, yt, at, w0, s, chains=1, want_w=False):
      asked.append((tuple(xt.shape), chains, s))
      return body(xt, yt, at, w0, s, chains=chains, want_w=want_w)
    _svm.svm_dca = watched
    try:
      kw = dict(chains_per_tile=sc.WORKERS // workers, dtype=dt)
      _, alpha_1 = _fit(x, y, 1, **kw)
      # one tile body per band and iteration, with the reference's scaled_lambda
      assert asked == [((sc.N // workers, sc.D), sc.WORKERS // workers, sc.WORKERS * 1.0 / (sc.LA * sc.N))] * workers
      w_3, alpha_3 = _fit(x, y, sc.ITERS, **kw)
    finally:
      _svm.svm_dca = body
    assert w_3.shape == (sc.D, 1) and alpha_3.shape == (sc.N, 1) and w_3.dtype == alpha_3.dtype == dt
    got = {'alpha_1': alpha_1, 'alpha_3': alpha_3, 'w_3': w_3}
    sc.check_accuracy(got, dt, '%s driver at %d workers' % (backend, workers))
    # the passes are the stated order's bytes: alpha of the whole run equals a run with the restated body
    alphas, _ = sc.run(sc.restated, x, y, dtype=dt)
    assert alpha_1.reshape(-1).tobytes() == alphas[0].tobytes()
    # the training accuracy is what the yardstick's w gives
    want_w = np.asarray(sc.golden_yardstick(dt)['w_3'], np.float64).reshape(sc.D, 1)
    labels = np.asarray(svm.predict_labels(sp.from_numpy(w_3), x.astype(dt)).glom())
    assert labels.shape == (sc.N, 1) and labels.dtype == np.int64
    acc = float((labels == y).mean())
    want_acc = float((np.where(x.astype(dt).astype(np.float64).dot(want_w) >= 0, 1, -1) == y).mean())
    print('training accuracy after %d iterations: %.3f (yardstick %.3f)' % (sc.ITERS, acc, want_acc))
    assert acc == want_acc
  finally:
    sp.shutdown()


@pytest.mark.parametrize('backend', BACKENDS)
def test_chains_per_tile_is_more_tiles(backend):
  """num_workers = 1, chains_per_tile = 4 gives the bytes of num_workers = 4, chains_per_tile = 1, for alpha: after one
  iteration, whose passes all start from w = 0 (the next iteration starts from w, a sum that each tiling forms in its
  own order)."""
  x, y = sc.golden_input()
  got = []
  for workers, chains in ((1, 4), (4, 1), (2, 2)):
    _start(backend, workers)
    try:
      got.append(_fit(x, y, 1, chains_per_tile=chains)[1])
    finally:
      sp.shutdown()
  assert got[0].any() and got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


@pytest.mark.parametrize('backend', BACKENDS)
def test_inputs_and_predictions(backend):
  x, y = sc.golden_input()
  _start(backend, 2)
  try:
    # T = 0: zeros, as a lazy expression
    w = svm.fit(x, y, T=0)
    assert isinstance(w, sp.expr.Expr) and not np.asarray(w.glom()).any() and np.asarray(w.glom()).shape == (sc.D, 1)
    w0, a0 = _fit(x.astype(np.float32), y, 0)
    assert w0.dtype == a0.dtype == np.float32 and not w0.any() and not a0.any() and a0.shape == (sc.N, 1)
    # labels (n,) of another dtype, data as arrays or expressions: the same bytes
    want_w, want_a = _fit(x, y, 2)
    for data, labels in ((x, y.reshape(-1)), (sp.from_numpy(x), sp.from_numpy(y.astype(np.float32))),
                         (x, y.reshape(-1).astype(np.int32))):
      got_w, got_a = _fit(data, labels, 2)
      assert got_w.tobytes() == want_w.tobytes() and got_a.tobytes() == want_a.tobytes()
    # float32 data runs in float32; integer data in float64; dtype forces
    assert _fit(x.astype(np.float32), y, 1)[0].dtype == np.float32
    assert _fit(np.round(x * 4).astype(np.int32), y, 1)[0].dtype == np.float64
    assert _fit(x, y, 1, dtype=np.float32)[0].dtype == np.float32
    # fit returns the lazy w of fit_state
    w = svm.fit(x, y, T=2, la=sc.LA)
    assert isinstance(w, sp.expr.Expr) and np.asarray(w.glom()).tobytes() == want_w.tobytes()
    # predictions: the sign of X w, 0 counted as +1
    scores = x.dot(want_w)
    labels = np.asarray(svm.predict_labels(w, x).glom())
    assert labels.tolist() == np.where(scores >= 0, 1, -1).tolist()
    for i in (0, 5, 77):
      assert svm.predict(w, x[i]) == svm.predict(w, sp.from_numpy(x[i:i + 1])) == (1 if scores[i, 0] >= 0 else -1)
    assert svm.predict(w, np.zeros(sc.D)) == 1
    assert (np.asarray(svm.predict_labels(w, x.astype(np.float32)).glom()) == labels).mean() > 0.98
  finally:
    sp.shutdown()


def test_refusals():
  x, y = sc.golden_input()
  _start('numpy', 2)
  try:
    for la in (0.0, -1.0, float('inf'), float('nan')):
      with pytest.raises(ValueError, match='la'):
        svm.fit(x, y, la=la)
    with pytest.raises(ValueError, match='T = -1'):
      svm.fit(x, y, T=-1)
    with pytest.raises(ValueError, match='chains_per_tile'):
      svm.fit(x, y, chains_per_tile=0)
    with pytest.raises(ValueError, match=r'\(n, d\)'):
      svm.fit(x.reshape(-1), y)
    with pytest.raises(ValueError, match='d = 4097'):
      svm.fit(np.zeros((2, 4097)), y[:2])
    with pytest.raises(ValueError, match='d = 0'):
      svm.fit(x[:, :0], y)
    for bad in (y[:-1], y.reshape(2, -1), np.concatenate([y, y], axis=1)):
      with pytest.raises(ValueError, match='labels of shape'):
        svm.fit(x, bad)
    for bad in (x.astype(np.complex128), x.astype(object)):
      with pytest.raises(TypeError, match='real'):
        svm.fit(bad, y)
    with pytest.raises(TypeError, match='real'):
      svm.fit(x, y.astype(np.complex64))
    with pytest.raises(TypeError, match='float32 float64'):
      svm.fit(x, y, dtype=np.float16)
    with pytest.raises(ValueError, match='predict_labels'):
      svm.predict_labels(np.zeros((sc.D + 1, 1)), x)
  finally:
    sp.shutdown()
