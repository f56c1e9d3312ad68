"""Records tests/golden/nbody_w4.npz: the reference's own n-body step (spartan/examples/nbody.py, move) on the small
galaxy of tests/nbody_cases.golden_input -- 24 bodies, SI units by random_galaxy's formulas, float64 -- at 4 workers,
3 moves of dt = one year, with the helpers of make_golden.py (the reference tree is copied to a scratch directory,
transliterated to Python 3 there and run in process; only the arrays are kept).

  python tests/golden/make_golden_nbody.py

  state0          the seven input arrays as a [7, 24] array in the order m, x, y, z, vx, vy, vz
  accel0          [3, 24]: the three sum(f, axis=0) of the first move, the expressions move hands to expr.sum's
                  caller, evaluated on their own (the script watches the module's `expr.sum`)
  state3          [7, 24]: the state after 3 moves
  as_written_vx   [24]: vx after one move of the reference's UNMODIFIED move (its set_diagonal as written); NaN
                  throughout if that move does not evaluate (the script prints what stopped it)
  whole_run       1 if the transliterated reference evaluated move; 0 if the script had to compose the arrays in NumPy
                  float64 (it prints what stopped it)

accel0 and state3 come from the reference's own move with nbody.set_diagonal replaced, in this script, by an
element-wise one: a map_with_location whose mapper sets the entries with row == column inside its tile.  The
reference's set_diagonal as written returns the bare scalar in place of a WHOLE tile when the tile's corner has
row == column.  Read as "the tile becomes the scalar" that zeroes every force at one worker and leaves 0 / 0 on the true
diagonal of the other bands at four; in the reference itself the map operator then asks the float for its shape and
the move raises AttributeError -- either way nothing one can keep, and as_written_vx records which of the two this
run saw.  Its docstring states the intent the replacement implements.

The script asserts that every pair is farther apart than 2 * rmin (rmin = 1 m) at every recorded step."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import nbody_cases as case  # noqa: E402

WORKERS = 4
MOVES = 3
KEYS = ('m', 'x', 'y', 'z', 'vx', 'vy', 'vz')
RMIN = 1.0


def _elementwise_mapper(tile, ex, scalar):
  """The entries of this tile with (global) row == column set to `scalar`."""
  ul = ex[0]
  out = np.array(tile)
  rows = ul[0] + np.arange(out.shape[0])
  cols = ul[1] + np.arange(out.shape[1])
  out[rows[:, None] == cols[None, :]] = scalar
  return out


def _stack(galaxy):
  return np.asarray([np.asarray(galaxy[k], np.float64) for k in KEYS])


class _Watched(object):
  """The reference's `expr` module with the results of `sum` kept."""

  def __init__(self, real):
    self.real, self.sums = real, []

  def __getattr__(self, name):
    return getattr(self.real, name)

  def sum(self, *args, **kw):
    node = self.real.sum(*args, **kw)
    self.sums.append(node)
    return node


def _composed_move(g, dt):
  """The reference's expression in NumPy float64, with the element-wise diagonal; returns the three sums."""
  dx, dy, dz = (-(g[k][None, :] - g[k][:, None]) for k in ('x', 'y', 'z'))
  r = np.sqrt(dx ** 2 + dy ** 2 + dz ** 2)
  np.fill_diagonal(r, 1.0)
  mask = r < 1.0
  r = r * ~mask + 1.0 * mask
  m = g['m'][:, None]
  sums = []
  for v, p, d in (('vx', 'x', dx), ('vy', 'y', dy), ('vz', 'z', dz)):
    f = case.G * m * d / r ** 3
    np.fill_diagonal(f, 0.0)
    sums.append(f.sum(axis=0))
    g[v] = g[v] + dt * sums[-1]
  for v, p in (('vx', 'x'), ('vy', 'y'), ('vz', 'z')):
    g[p] = g[p] + dt * g[v]
  return np.asarray(sums)


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  mg.install_stubs()
  sp = mg.import_reference()
  start = case.golden_input()
  n = len(start['m'])
  dt = case.YEAR
  out = {'state0': _stack(start)}
  assert case.min_separation(start) > 2 * RMIN

  def galaxy():
    return {k: sp.from_numpy(np.array(start[k]), tile_hint=(n // WORKERS,)) for k in KEYS}

  def host(g):
    return {k: np.asarray(g[k].glom(), np.float64).reshape(n) for k in KEYS}

  whole = 1
  try:
    mg.start_cluster(sp, WORKERS)
    from spartan.config import FLAGS
    FLAGS.num_workers = WORKERS
    import spartan
    from spartan.examples import nbody as ref
    assert ref.G == case.G and ref.dt == dt
    as_written_set_diagonal = ref.set_diagonal
    # with the element-wise diagonal
    ref.set_diagonal = lambda array, scalar: spartan.map_with_location(array, _elementwise_mapper, fn_kw={'scalar': scalar})
    g = galaxy()
    states = []
    ref.expr = watched = _Watched(ref.expr)
    for _ in range(MOVES):
      ref.move(g, dt)
      states.append(host(g))
    accel0 = np.asarray([np.asarray(node.glom(), np.float64).reshape(n) for node in watched.sums[:3]])
    print('nbody_w4.npz: move() evaluated at %d workers' % WORKERS)
    # ... and the reference as written, one move (last: whatever it does to the cluster, nothing runs after it)
    ref.set_diagonal = as_written_set_diagonal
    try:
      g = galaxy()
      ref.move(g, dt)
      with np.errstate(all='ignore'):
        as_written = host(g)['vx']
    except Exception as e:   # noqa: BLE001
      print('nbody_w4.npz: move() with set_diagonal AS WRITTEN did not evaluate (as_written_vx is NaN):',
            type(e).__name__, str(e)[:200])
      as_written = np.full(n, np.nan)
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    print("nbody_w4.npz: the reference's move() did not evaluate:", type(e).__name__, str(e)[:400])
    whole = 0
    as_written = np.full(n, np.nan)
    g = {k: np.array(start[k]) for k in KEYS}
    states, sums = [], []
    for _ in range(MOVES):
      sums.append(_composed_move(g, dt))
      states.append({k: g[k].copy() for k in KEYS})
    accel0 = sums[0]

  for s in states:
    assert all(np.isfinite(s[k]).all() for k in KEYS)
    sep = case.min_separation(s)
    assert sep > 2 * RMIN, sep
  composed = {k: np.array(start[k]) for k in KEYS}
  np.testing.assert_allclose(accel0, _composed_move(composed, dt), rtol=1e-9, atol=0)
  np.testing.assert_allclose([states[0][k] for k in KEYS], [composed[k] for k in KEYS], rtol=1e-9, atol=0)
  out.update(accel0=accel0, state3=_stack(states[-1]), as_written_vx=np.asarray(as_written, np.float64),
             whole_run=np.asarray(whole, np.int64))
  print('nbody_w4.npz: the closest pair is %.3g m apart after %d moves; as written, vx after one move is %s'
        % (case.min_separation(states[-1]), MOVES, np.array2string(out['as_written_vx'][:8], precision=3)))
  path = os.path.join(HERE, 'nbody_w4.npz')
  np.savez_compressed(path, **out)
  print('nbody_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out))


if __name__ == '__main__':
  main()
