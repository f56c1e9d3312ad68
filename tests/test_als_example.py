"""examples/als: the alternating-least-squares driver.  CPU leg: the host framework on the injected NumPy backend, where
the tile body is the NumPy restatement beside the driver (examples/_als.py).  GPU leg: the same checks on the HIP
backend (sp_als_solve).

Input: 24 x 40 integer ratings in 0 .. 4 (user row 3 rated nothing, every item is rated), 6 features, la = 0.065,
alpha = 40.  Yardstick: tests/golden/als_w4.npz, the outputs of the reference's own tile body (a loop over rows around
scipy.linalg.lstsq, float64) chained over two iterations from M0, recorded by tests/golden/make_golden_als.py.

Stepwise: each half-step of ours, started from the golden's input of that step, matches the golden's output within
TWICE the derived bound of tests/als_cases.py for that step's operands in the dtype under test -- both sides carry
rounding error in float64; in float32 the second share covers the rounding of the float64 operands to float32, at most
one more rounding per factor, which the bound's gamma_{t+3} |Y|^T |W| |Y| term dominates.
Wiring: als(A, M=M0, num_iter=2) equals our own chained als_solve calls bit for bit, at 1 worker and at 4 with A in
four row bands (a row's result does not depend on the rows solved with it).
Objective: in explicit mode in float64 the regularised objective
  sum_{r != 0} (r - u . m)^2 + la (sum_i |S_i| |u_i|^2 + sum_j |S_j| |m_j|^2)
does not increase over any half-step, up to a relative 1e-10: each half-step minimises it exactly over its factor, and
the slack covers the rounding of the evaluation.  Measured figures are printed before each assertion."""
import functools
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples import _als
from spartan_amd.examples.als import als
from tests import als_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
USERS, ITEMS, F, SEED = 24, 40, 6, 20150714
LA, ALPHA = ac.LA, ac.ALPHA
MODES = (('explicit', False), ('implicit', True))
STEPS = (('U1', False, 'M0'), ('M1', True, 'U1'), ('U2', False, 'M1'), ('M2', True, 'U2'))   # (output, transposed?, input)


@functools.lru_cache(maxsize=None)
def ratings():
  rng = np.random.RandomState(SEED)
  a = rng.randint(0, 5, size=(USERS, ITEMS)).astype(np.int32)
  a[3] = 0
  assert np.all((a != 0).sum(axis=0) > 0)
  a.setflags(write=False)
  return a


@functools.lru_cache(maxsize=None)
def start_factors():
  a = ratings()
  m0 = np.random.RandomState(SEED + 1).rand(ITEMS, F)
  m0[:, 0] = a.sum(axis=0) * 1.0 / np.count_nonzero(a, axis=0)
  m0.setflags(write=False)
  return m0


@functools.lru_cache(maxsize=None)
def golden():
  g = dict(np.load(os.path.join(HERE, 'golden', 'als_w4.npz')))
  assert g['A'].tobytes() == ratings().tobytes() and g['M0'].tobytes() == start_factors().tobytes()
  return g


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _host(be, t):
  return np.array(be.to_numpy(t))


def _chain(be, dtype, implicit):
  """Our own four half-steps from M0, as host arrays."""
  a = ratings().astype(dtype)
  out = {'M0': start_factors().astype(dtype)}
  for name, transposed, src in STEPS:
    r = np.ascontiguousarray(a.T if transposed else a)
    out[name] = _host(be, _als.als_solve(be.from_numpy(r), be.from_numpy(out[src]), LA, ALPHA, implicit))
  return out


def _check_stepwise(backend, dtype):
  g = golden()
  ctx = _start(backend, 1)
  try:
    be = ctx.backend
    a = ratings().astype(dtype)
    for mode, implicit in MODES:
      for name, transposed, src in STEPS:
        r = np.ascontiguousarray(a.T if transposed else a)
        y = (g['M0'] if src == 'M0' else g['%s_%s' % (mode, src)]).astype(dtype)
        info = be.zeros((1,), np.int32)
        got = _host(be, _als.als_solve(be.from_numpy(r), be.from_numpy(y), LA, ALPHA, implicit, info=info))
        assert got.dtype == np.dtype(dtype) and int(_host(be, info)[0]) == 0
        _, bound, _ = ac.oracle(r, y, LA, ALPHA, implicit)
        ac.check(got, g['%s_%s' % (mode, name)], bound, 'als %s %s %s %s' % (backend, np.dtype(dtype).name, mode, name),
                 scale=2.0)
        if not implicit and not transposed:
          assert not np.any(got[3])               # the user who rated nothing
  finally:
    sp.shutdown()


def _check_wiring(backend, workers, dtype, implicit):
  ctx = _start(backend, workers)
  try:
    a = ratings()
    A = sp.from_numpy(a, tile_hint=(USERS // workers, ITEMS)) if workers > 1 else sp.from_numpy(a)
    U, M = als(A, la=LA, alpha=ALPHA, implicit_feedback=implicit, num_features=F, num_iter=2,
               M=np.array(start_factors()), dtype=dtype)
    assert tuple(U.shape) == (USERS, F) and tuple(M.shape) == (ITEMS, F)
    u, m = np.asarray(U.glom()), np.asarray(M.glom())
    ours = _chain(ctx.backend, dtype, implicit)
    assert u.dtype == np.dtype(dtype) and m.dtype == np.dtype(dtype)
    assert u.tobytes() == ours['U2'].tobytes() and m.tobytes() == ours['M2'].tobytes()
    return u, m
  finally:
    sp.shutdown()


def _objective(a, u, m):
  rated = a != 0
  resid = np.where(rated, a - u.dot(m.T), 0.0)
  return float((resid ** 2).sum() + LA * ((rated.sum(axis=1) * (u ** 2).sum(axis=1)).sum()
                                          + (rated.sum(axis=0) * (m ** 2).sum(axis=1)).sum()))


def _check_objective(backend):
  ctx = _start(backend, 1)
  try:
    c = _chain(ctx.backend, np.float64, False)
  finally:
    sp.shutdown()
  a = ratings().astype(np.float64)
  values = [_objective(a, c[u], c[m]) for u, m in (('U1', 'M0'), ('U1', 'M1'), ('U2', 'M1'), ('U2', 'M2'))]
  print('als %s: objective after each half-step: %s' % (backend, ' '.join('%.12g' % v for v in values)))
  for before, after in zip(values, values[1:]):
    assert after <= before * (1 + 1e-10)
  assert values[-1] < values[0]


def _check_refusals(backend):
  ctx = _start(backend, 1)
  try:
    a, m0 = np.array(ratings()), np.array(start_factors())
    with pytest.raises(ValueError, match='la'):
      als(sp.from_numpy(a), la=0, M=m0, num_features=F)
    with pytest.raises(ValueError, match='64'):
      als(sp.from_numpy(a), num_features=65)
    with pytest.raises(ValueError, match='M of shape'):
      als(sp.from_numpy(a), M=m0, num_features=F + 1)
    bad = a.copy()
    bad[7, 11] = -500                                  # alpha r y y^T outweighs everything else in row 7's system
    U, M = als(sp.from_numpy(bad), implicit_feedback=True, num_features=F, num_iter=1, M=m0)
    with pytest.raises(np.linalg.LinAlgError, match='positive definite'):
      U.glom()
    # the default start (rand, column 0 the average rating) runs and every system is definite
    U, M = als(sp.from_numpy(a), num_features=F, num_iter=1)
    u, m = np.asarray(U.glom()), np.asarray(M.glom())
    assert u.shape == (USERS, F) and m.shape == (ITEMS, F) and np.all(np.isfinite(u)) and np.all(np.isfinite(m))
    assert not np.any(u[3])
  finally:
    sp.shutdown()


def test_the_golden_holds_the_reference_run():
  g = golden()
  for mode, _ in MODES:
    for name, transposed, _ in STEPS:
      assert g['%s_%s' % (mode, name)].shape == ((ITEMS if transposed else USERS), F)
    assert not np.any(g[mode + '_U1'][3])
    if mode + '_als_U' in g:                           # the reference's whole als() at 4 workers from the same M0
      for whole, step in (('_als_U', '_U2'), ('_als_M', '_M2')):
        err = ac.errors(g[mode + whole], g[mode + step])
        print('golden %s: max row error of als()%s against the chained %s = %.3g' % (mode, whole, step, err.max()))
        assert err.max() <= 1e-9


def test_stepwise_against_the_reference_cpu():
  _check_stepwise('numpy', np.float64)


@pytest.mark.parametrize('workers', (1, 4))
@pytest.mark.parametrize('mode', MODES, ids=lambda m: m[0])
def test_the_driver_is_the_chain_of_its_half_steps_cpu(mode, workers):
  _check_wiring('numpy', workers, np.float64, mode[1])


def test_float32_driver_cpu():
  _check_wiring('numpy', 4, np.float32, False)
  _check_wiring('numpy', 1, np.float32, True)


def test_the_objective_does_not_increase_cpu():
  _check_objective('numpy')


def test_refusals_cpu():
  _check_refusals('numpy')


# ---- the same on the device ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_stepwise_against_the_reference_gpu(dtype):
  _check_stepwise('hip', dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('workers', (1, 4))
@pytest.mark.parametrize('mode', MODES, ids=lambda m: m[0])
def test_the_driver_is_the_chain_of_its_half_steps_gpu(mode, workers):
  _check_wiring('hip', workers, np.float64, mode[1])
  if workers == 4:
    _check_wiring('hip', workers, np.float32, mode[1])


@pytest.mark.gpu
def test_the_objective_does_not_increase_gpu():
  _check_objective('hip')


@pytest.mark.gpu
def test_refusals_gpu():
  _check_refusals('hip')
