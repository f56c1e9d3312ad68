"""examples/nbody: the n-body driver.  CPU leg: the host framework on the injected NumPy backend, where the tile body is
the NumPy restatement beside the driver (examples/_nbody.py).  GPU leg: the same checks on the HIP backend
(sp_nbody_accel), called from tests/test_nbody_gpu.py.

Input and yardstick: tests/golden/nbody_w4.npz, recorded by tests/golden/make_golden_nbody.py from the reference's own
move at 4 workers on the 24 bodies of tests/nbody_cases.golden_input (SI units, float64, 3 moves of a year), with the
reference's set_diagonal replaced by an element-wise one -- the deviation the driver's docstring begins with;
`as_written_vx` in the same file records what the reference's move does as written.

Every comparison is against the first-order bounds of tests/nbody_cases.trajectory: ours against the oracle within the
bound of our dtype, ours against the golden within the sum of our bound and the reference's (float64).  The velocities
after the first move from rest are dt * a, so the recorded sums `accel0` are compared with v / dt.  The measured share
of every bound is printed before it is asserted."""
import functools
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples import _nbody, nbody
from tests import nbody_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ('m', 'x', 'y', 'z', 'vx', 'vy', 'vz')
MOVES = 3
UNIT_N, UNIT_STEP = 24, 1e-3


@functools.lru_cache(maxsize=None)
def golden():
  g = dict(np.load(os.path.join(HERE, 'golden', 'nbody_w4.npz')))
  start = nc.golden_input()
  assert g['state0'].tobytes() == np.asarray([start[k] for k in KEYS]).tobytes()
  return g


def unit_galaxy(dtype):
  x, y, z, mass = nc.unit_case(UNIT_N, dtype)
  zero = np.zeros(UNIT_N, np.dtype(dtype))
  return {'m': mass, 'x': x, 'y': y, 'z': z, 'vx': zero, 'vy': zero.copy(), 'vz': zero.copy()}


@functools.lru_cache(maxsize=None)
def path(which, dtype):
  """The oracle's trajectory and bounds (nbody_cases.trajectory) of the golden galaxy ('si') or the unit-scale one."""
  if which == 'si':
    out = nc.trajectory(nc.golden_input(), MOVES, nc.YEAR, nc.G, 1.0, dtype)
    rmin = 1.0
  else:
    out = nc.trajectory(unit_galaxy(dtype), MOVES, UNIT_STEP, nc.UNIT_G, nc.UNIT_RMIN, dtype)
    rmin = nc.UNIT_RMIN
  for state, _ in out:                         # the cap holds along the whole path
    nc.assert_clear_of_rmin(state['x'], state['y'], state['z'], rmin)
  return out


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _distributed(galaxy, workers):
  n = len(galaxy['m'])
  return {k: sp.from_numpy(np.array(v), tile_hint=(-(-n // workers),)) for k, v in galaxy.items()}


def _host(galaxy):
  return {k: np.asarray(galaxy[k].glom()) for k in KEYS}


def _check_state(got, entry, label, dtype, against=None, extra=None):
  """|got - oracle| within the bound of `entry` = (state, bound); with `against` (a state of the reference) and `extra`
  (its bound), |got - against| within the sum of the two."""
  state, bound = entry
  worst = 0.0
  for key in KEYS[1:]:
    e = bound['x'] if key in 'xyz' else bound['v']
    assert got[key].dtype == np.dtype(dtype), (key, got[key].dtype)
    worst = max(worst, nc.share(np.abs(np.asarray(got[key], nc.LD) - state[key]), e))
    if against is not None:
      e2 = e + (extra['x'] if key in 'xyz' else extra['v'])
      worst = max(worst, nc.share(np.abs(np.asarray(got[key], nc.LD) - np.asarray(against[key], nc.LD)), e2))
  print('%s: at %.3g of the trajectory bounds' % (label, worst))
  assert worst <= 1.0, label
  return worst


def run_moves(backend, workers, dtype, method, which='si'):
  """The states after every move (host dicts), what the tile body was asked, and what was allocated."""
  dt = np.dtype(dtype)
  start = nc.golden_input() if which == 'si' else unit_galaxy(dt)
  kw = dict(method=method) if which == 'si' else dict(method=method, g=nc.UNIT_G, rmin=nc.UNIT_RMIN)
  step = nc.YEAR if which == 'si' else UNIT_STEP
  n = len(start['m'])
  ctx = _start(backend, workers)
  try:
    galaxy = _distributed({k: np.asarray(v, dt) for k, v in start.items()}, workers)
    asked, allocated = [], []
    body = _nbody.nbody_accel

    def watched(x, y, z, mass, r0, m, **kw):
      asked.append((int(r0), int(m), tuple(np.shape(x))))
      return body(x, y, z, mass, r0, m, **kw)
    _nbody.nbody_accel = watched
    on_backend = []
    real = getattr(ctx.backend, 'nbody_accel', None)
    if real is not None:
      def watched_backend(x, y, z, mass, r0, m, **kw):
        on_backend.append((int(r0), int(m)))
        return real(x, y, z, mass, r0, m, **kw)
      ctx.backend.nbody_accel = watched_backend
    empty = getattr(ctx.backend, 'empty', None)
    if empty is not None:
      def watched_empty(shape, dtype):
        allocated.append(tuple(shape))
        return empty(shape, dtype)
      ctx.backend.empty = watched_empty
    states = []
    try:
      for s in range(MOVES):
        if s == 0:
          nbody.move(galaxy, step, **kw)
        else:
          nbody.simulate(galaxy, 1, dt=step, **kw)
        states.append(_host(galaxy))
    finally:
      _nbody.nbody_accel = body
      if real is not None:
        del ctx.backend.nbody_accel
      if empty is not None:
        del ctx.backend.empty
    if real is not None and method == 'fused':
      assert sorted(on_backend) == sorted(a[:2] for a in asked)
    return states, asked, allocated, n
  finally:
    sp.shutdown()


def check_driver(backend, workers, dtype, method='fused', which=None):
  dt = np.dtype(dtype)
  which = which or ('si' if dt == np.float64 else 'unit')
  states, asked, allocated, n = run_moves(backend, workers, dt, method, which)
  label = 'nbody %s %s %d workers %s %s' % (backend, method, workers, dt.name, which)
  band = -(-n // workers)
  if method == 'fused':
    # the tile body is asked once per band and move, with (r0, m) of that band and the four (n,) arrays
    assert sorted(asked) == sorted([(lo, min(band, n - lo), (n,)) for lo in range(0, n, band)] * MOVES), asked
    assert not [s for s in allocated if len(s) == 2 and min(s) >= band and max(s) >= n], allocated   # nothing n x n
  else:
    assert not asked
  ours = path(which, dt.name)
  g = golden() if which == 'si' else None
  theirs = path('si', 'float64') if which == 'si' else None
  # the first move from rest: v = dt a, against the oracle and against the reference's recorded sums
  first = None
  if g is not None:
    first = {k: np.zeros(n) for k in KEYS}
    for c, v in enumerate(('vx', 'vy', 'vz')):
      first[v] = np.float64(nc.YEAR) * g['accel0'][c]
    for p, v in (('x', 'vx'), ('y', 'vy'), ('z', 'vz')):
      first[p] = nc.golden_input()[p] + np.float64(nc.YEAR) * first[v]
  _check_state(states[0], ours[1], label + ' accel0', dt, first, theirs[1][1] if theirs else None)
  last = None if g is None else dict(zip(KEYS, g['state3']))
  _check_state(states[-1], ours[MOVES], label + ' state3', dt, last, theirs[MOVES][1] if theirs else None)
  return states


def check_workers_agree(backend, dtype=np.float64):
  one = run_moves(backend, 1, dtype, 'fused')[0][-1]
  four = run_moves(backend, 4, dtype, 'fused')[0][-1]
  bound = path('si', np.dtype(dtype).name)[MOVES][1]
  for key in KEYS[1:]:
    if backend == 'hip':
      assert one[key].tobytes() == four[key].tobytes(), key      # a band alone gives the bits of the whole
    e = bound['x'] if key in 'xyz' else bound['v']
    assert nc.share(np.abs(np.asarray(one[key], nc.LD) - np.asarray(four[key], nc.LD)), 2 * e) <= 1.0, key


def check_refusals(backend):
  start = {k: np.array(v) for k, v in nc.golden_input().items()}
  _start(backend, 4)
  try:
    def fresh(**changes):
      g = _distributed(start, 4)
      g.update(changes)
      return g
    with pytest.raises(ValueError, match='method'):
      nbody.move(fresh(), nc.YEAR, method='tree')
    for rmin in (0.0, -1.0, float('nan'), float('inf')):
      with pytest.raises(ValueError, match='rmin'):
        nbody.move(fresh(), nc.YEAR, rmin=rmin)
    for g in (float('nan'), float('inf')):
      with pytest.raises(ValueError, match='g = '):
        nbody.move(fresh(), nc.YEAR, g=g)
      with pytest.raises(ValueError, match='g = '):
        nbody.move(fresh(), nc.YEAR, method='expr', g=g)
    with pytest.raises(ValueError, match='1-D and of equal length'):
      nbody.move(fresh(vy=np.zeros(23)), nc.YEAR)
    with pytest.raises(ValueError, match='1-D and of equal length'):
      nbody.move({k: v.reshape(24, 1) for k, v in start.items()}, nc.YEAR)
    missing = fresh()
    del missing['vz']
    with pytest.raises(KeyError, match='vz'):
      nbody.move(missing, nc.YEAR)
    for bad in (start['x'].astype(np.complex128), start['x'].astype(object)):
      with pytest.raises(TypeError, match='real numbers'):
        nbody.move(fresh(x=bad), nc.YEAR)
    # integer arrays are converted to float64; NumPy arrays are taken as they are
    whole = {k: (np.arange(24) * 3 % 7 + 1) * (10 if k == 'm' else 1) if k in 'mxyz' else np.zeros(24, np.int64) for k in KEYS}
    whole['z'] = np.arange(24)
    ints = {k: v.astype(np.int32) for k, v in whole.items()}
    floats = {k: v.astype(np.float64) for k, v in whole.items()}
    nbody.move(ints, 0.5, g=1.0, rmin=0.5)
    nbody.move(floats, 0.5, g=1.0, rmin=0.5)
    for k in KEYS:
      a, b = np.asarray(ints[k].glom()), np.asarray(floats[k].glom())
      assert a.dtype == np.float64 and a.tobytes() == b.tobytes(), k
  finally:
    sp.shutdown()


def test_the_golden_holds_the_reference_run():
  g = golden()
  assert int(g['whole_run']) == 1                      # accel0 and state3 are the reference's own move
  ref = path('si', 'float64')
  a, s = ref[1][0]['a'], None
  want = nc.oracle(*(nc.golden_input()[k] for k in ('x', 'y', 'z', 'm')), nc.G, 1.0)
  sh = nc.share(np.abs(np.asarray(g['accel0'], nc.LD) - want[0]), nc.gamma(24, np.float64) * want[1])
  print("the reference's accel0 against the oracle: %.3g of gamma * sum|t|" % sh)
  assert sh <= 1.0 and np.array_equal(a, want[0])
  _check_state(dict(zip(KEYS, g['state3'])), ref[MOVES], "the reference's state3", np.float64)
  # what the reference's set_diagonal does as written: nothing finite, or zeros in the first band
  w = g['as_written_vx']
  assert not np.isfinite(w).all() or not w[:6].any()


@pytest.mark.parametrize('method', nbody.METHODS)
@pytest.mark.parametrize('workers', (1, 3, 4))
def test_the_driver_reproduces_the_reference_cpu(workers, method):
  check_driver('numpy', workers, np.float64, method)


@pytest.mark.parametrize('method', nbody.METHODS)
def test_float32_on_the_unit_scale_case_cpu(method):
  check_driver('numpy', 4, np.float32, method)


def test_one_and_four_workers_agree_cpu():
  check_workers_agree('numpy')


def test_refusals_cpu():
  check_refusals('numpy')


def test_the_interface_of_the_reference():
  assert (nbody.G, nbody.dt, nbody.r_ly, nbody.m_sol) == (6.67384e-11, 60 * 60 * 24 * 365.25, 9.4607e15, 1.9891e30)
  _start('numpy', 2)
  try:
    galaxy = nbody.random_galaxy(10)
    assert sorted(galaxy) == sorted(KEYS)
    nbody.simulate(galaxy, 2)
    after = _host(galaxy)
    assert all(v.dtype == np.float64 and v.shape == (10,) and np.isfinite(v).all() for v in after.values())
    assert after['vx'].any() and (after['m'] >= nbody.m_sol).all()
  finally:
    sp.shutdown()
