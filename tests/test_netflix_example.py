"""examples/netflix: the SGD matrix factorisation driver.  CPU leg: the host framework on the injected NumPy backend,
where the tile body is the NumPy restatement beside the driver (examples/_netflix.py).  GPU leg (marked): the same
checks on the HIP backend (sp_sgd_mf).

Input and reference: tests/golden/netflix_w4.npz, recorded by tests/golden/make_golden_netflix.py from the reference's
own sgd at 4 workers (52 x 400 on a 4 x 4 grid, rank 20, float32, two epochs, each with the strata the reference
drew).  Accuracy: the rule of tests/netflix_cases.py -- U and M after either epoch within 8 e_ref of the float64
yardstick (8 e_ref / 2^29 in float64); every ratio is printed before it is asserted."""
import numpy as np
import pytest
import scipy.sparse as sps

import spartan_amd as sp
from spartan_amd.examples import _netflix, netflix
from tests import netflix_cases as nc

BACKENDS = ('numpy', pytest.param('hip', marks=pytest.mark.gpu))
DTYPES = (np.float32, np.float64)


def _start(backend, workers=nc.WORKERS):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _loader(inputs, ex, whole=None):
  yield ex, whole[ex.ul[0]:ex.lr[0], ex.ul[1]:ex.lr[1]].tocoo()


def _arrays(dtype=np.float32, v_dtype=None):
  """(V, M, U) of the golden input on its 4 x 4 grid, the factors in `dtype`."""
  rows, cols, vals, u0, m0 = nc.golden_input()
  whole = sps.csr_matrix((vals.astype(v_dtype or dtype), (rows, cols)), shape=(nc.USERS, nc.MOVIES))
  hint = (-(-nc.USERS // nc.GRID), -(-nc.MOVIES // nc.GRID))
  V = sp.sparse_empty((nc.USERS, nc.MOVIES), tile_hint=hint, dtype=v_dtype or dtype)
  V = sp.eager(sp.tocoo(sp.shuffle(V, _loader, target=V, kw={'whole': whole})))
  M = sp.eager(sp.from_numpy(m0.astype(dtype), tile_hint=(hint[1], nc.RANK)))
  U = sp.eager(sp.from_numpy(u0.astype(dtype), tile_hint=(hint[0], nc.RANK)))
  return V, M, U


def _glom(a):
  return np.asarray(sp.evaluate(a).glom() if hasattr(a, 'evaluate') else a.glom())


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('backend', BACKENDS)
def test_the_golden_run(backend, dtype):
  dt = np.dtype(dtype)
  rows, cols, vals, u0, m0 = nc.golden_input()
  strata = nc.golden_strata()
  _start(backend)
  try:
    V, M, U = _arrays(dt)
    asked, body = [], _netflix.sgd_mf

    def watched(v, u, m, lr=None, want_error=False):
      asked.append((tuple(v.shape), tuple(u.shape), tuple(m.shape)))
      return body(v, u, m, lr=lr, want_error=want_error)
    _netflix.sgd_mf = watched
    got = []
    try:
      for t in range(nc.EPOCHS):
        step = netflix.sgd(V, M, U, strata=strata[t])
        assert step.strata == strata[t]
        assert step.evaluate() is step
        got.append((_glom(U), _glom(M)))         # M and U are updated in place
    finally:
      _netflix.sgd_mf = body
    assert sorted(asked) == sorted([((13, 100), (13, nc.RANK), (100, nc.RANK))] * 16 * nc.EPOCHS)     # one tile body per block and epoch
    assert got[0][0].dtype == got[0][1].dtype == dt and got[0][0].shape == u0.shape and got[0][1].shape == m0.shape
    nc.check_accuracy(got, dt, '%s driver' % backend)
    # the passes are the stated order's bytes
    want = nc.epochs(nc.restated, rows, cols, vals, u0, m0, strata, dtype=dt)
    for t in range(nc.EPOCHS):
      assert got[t][0].tobytes() == want[t][0].tobytes() and got[t][1].tobytes() == want[t][1].tobytes()
  finally:
    sp.shutdown()


@pytest.mark.parametrize('backend', BACKENDS)
def test_default_strata_want_error_lr_and_force(backend):
  rows, cols, vals, u0, m0 = nc.golden_input()
  assert netflix.default_strata(4, 4) == nc.default_strata(4, 4)
  assert netflix.default_strata(2, 3) == [[(0, 0), (1, 1)], [(0, 1), (1, 2)], [(0, 2), (1, 0)]]
  for gr, gc in ((1, 1), (2, 3), (5, 2), (4, 4)):
    strata = netflix.default_strata(gr, gc)
    assert netflix.check_strata(strata, gr, gc) == strata and len(strata) == max(gr, gc)
  _start(backend)
  try:
    V, M, U = _arrays()
    step = netflix.sgd(V, M, U, want_error=True)
    assert step.strata == nc.default_strata(4, 4) and step.error is None
    step.force()
    want_u, want_m = nc.epochs(nc.restated, rows, cols, vals, u0, m0, [nc.default_strata(4, 4)], n_epochs=1)[0]
    assert _glom(U).tobytes() == want_u.tobytes() and _glom(M).tobytes() == want_m.tobytes()
    # the sum of |d| over the epoch: each block's terms as the sequence sees them
    total, (u, m) = 0.0, (u0.copy(), m0.copy())
    rcuts, ccuts = nc.grid_cuts(nc.USERS, 4), nc.grid_cuts(nc.MOVIES, 4)
    for stratum in nc.default_strata(4, 4):
      for bi, bj in stratum:
        (r0, r1), (c0, c1) = rcuts[bi], ccuts[bj]
        un, mn, err = nc.restated(*nc.block(rows, cols, vals, rcuts[bi], ccuts[bj], np.float32), u[r0:r1], m[c0:c1])
        u[r0:r1], m[c0:c1] = un, mn
        total += float(err.astype(np.float64).sum())
    print('sum of |d| over the epoch: %r (float64 sum of the restated terms %r)' % (step.error, total))
    assert abs(step.error - total) <= 1442 * 2.0 ** -23 * total       # (a float32 sum of 1442 terms, any order)
    # lr: another step size, the same sequence
    V, M, U = _arrays()
    netflix.sgd(V, M, U, lr=1e-3).evaluate()
    want_u, _ = nc.epochs(lambda *a: nc.restated(*a[:5], lr=1e-3), rows, cols, vals, u0, m0, [nc.default_strata(4, 4)],
                          n_epochs=1)[0]
    assert _glom(U).tobytes() == want_u.tobytes()
    # float32 ratings under float64 factors are converted once
    V, M, U = _arrays(np.float64, v_dtype=np.float32)
    netflix.sgd(V, M, U, dtype=np.float64).evaluate()
    want_u, _ = nc.epochs(nc.restated, rows, cols, vals, u0, m0, [nc.default_strata(4, 4)], n_epochs=1, dtype=np.float64)[0]
    assert _glom(U).tobytes() == want_u.tobytes()
  finally:
    sp.shutdown()


@pytest.mark.parametrize('backend', BACKENDS)
def test_the_fake_loader_and_one_worker(backend):
  """The reference's test program: fake_netflix_mapper fills V (with duplicates and zeros), two epochs run."""
  _start(backend, 2)
  try:
    users, movies, r, d = 40, 300, 20, 3
    np.random.seed(5)
    V = sp.sparse_empty((users, movies), tile_hint=(-(-users // d), -(-movies // d)), dtype=np.float32)
    V = sp.eager(sp.tocoo(sp.shuffle(V, netflix.fake_netflix_mapper, target=V, kw={'p_rating': 400.0 / (users * movies)})))
    M = sp.eager(sp.rand(movies, r).astype(np.float32))
    U = sp.eager(sp.rand(users, r).astype(np.float32))
    u_before = _glom(U).copy()
    whole = sps.csr_matrix(V.glom())
    assert 0 < whole.nnz <= 9 * 44
    for _ in range(2):
      _ = netflix.sgd(V, M, U).evaluate()
    assert np.isfinite(_glom(U)).all() and np.isfinite(_glom(M)).all() and not np.array_equal(_glom(U), u_before)
  finally:
    sp.shutdown()


def test_refusals():
  _start('numpy')
  try:
    V, M, U = _arrays()
    rows, cols, vals, u0, m0 = nc.golden_input()
    good = nc.default_strata(4, 4)
    for bad, match in (([s[:-1] for s in good], 'miss'), (good + [[(0, 0)]], 'twice'), ([good[0] + good[1]] + good[2:], 'overlap'),
                       (good[:-1] + [good[-1][:-1] + [(4, 0)]], 'outside'), ([[1, 2]], 'list of lists'),
                       ([[(0, 0), (0, 1)]], 'overlap')):
      with pytest.raises(ValueError, match=match):
        netflix.sgd(V, M, U, strata=bad)
    with pytest.raises(TypeError, match='V must be a sparse'):
      netflix.sgd(sp.eager(sp.from_numpy(np.zeros((nc.USERS, nc.MOVIES), np.float32))), M, U)
    with pytest.raises(TypeError, match='V must be a sparse'):
      netflix.sgd(np.zeros((nc.USERS, nc.MOVIES), np.float32), M, U)
    with pytest.raises(ValueError, match='U of shape'):
      netflix.sgd(V, M, sp.eager(sp.from_numpy(u0[:-1])))
    with pytest.raises(ValueError, match='M of shape'):
      netflix.sgd(V, sp.eager(sp.from_numpy(m0[:, :-1])), U)
    with pytest.raises(ValueError, match='U of shape'):
      netflix.sgd(V, U, M)                           # (the factors swapped)
    with pytest.raises(ValueError, match='V must be 2-D'):
      netflix.sgd(type('Flat', (), dict(sparse=True, tiles={}, shape=(30,), dtype=np.float32))(), M, U)   # (sparse arrays are 2-D)
    for bad in (np.int64, np.int32):
      with pytest.raises(TypeError, match='astype'):
        netflix.sgd(V, M, sp.eager(sp.from_numpy(u0.astype(bad))))
    with pytest.raises(TypeError, match='astype'):
      netflix.sgd(V, sp.eager(sp.from_numpy(m0.astype(np.float64))), U)
    with pytest.raises(TypeError, match='dtype = float64'):
      netflix.sgd(V, M, U, dtype=np.float64)
    with pytest.raises(TypeError, match='float32 float64'):
      netflix.sgd(V, M, U, dtype=np.int32)
    with pytest.raises(ValueError, match='rank r = 513'):
      netflix.sgd(V, sp.eager(sp.from_numpy(np.zeros((nc.MOVIES, 513), np.float32), tile_hint=(100, 513))),
                  sp.eager(sp.from_numpy(np.zeros((nc.USERS, 513), np.float32), tile_hint=(13, 513))))
    with pytest.raises(ValueError, match='rank r = 0'):
      netflix.sgd(V, M, sp.eager(sp.from_numpy(np.zeros((nc.USERS, 0), np.float32))))
    with pytest.raises(ValueError, match='tiling of U cuts the rank'):
      netflix.sgd(V, M, sp.eager(sp.from_numpy(u0, tile_hint=(13, 10))))
    with pytest.raises(ValueError, match='tiling of M cuts the rank'):
      netflix.sgd(V, sp.eager(sp.from_numpy(m0, tile_hint=(100, 5))), U)
    for lr in (float('nan'), float('inf')):
      with pytest.raises(ValueError, match='lr'):
        netflix.sgd(V, M, U, lr=lr)
    # nothing was touched
    assert _glom(U).tobytes() == u0.tobytes() and _glom(M).tobytes() == m0.tobytes()
  finally:
    sp.shutdown()
