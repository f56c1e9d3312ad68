"""All-pairs gravity (interface of the reference's spartan/examples/nbody.py: `random_galaxy(n)`, `move(galaxy, dt)`,
`simulate(galaxy, timesteps)` and the constants G, dt, r_ly, m_sol; its tests/benchmark_nbody.py runs 1000 bodies for
50 steps).

A move, with the galaxy a dict of seven (n,) arrays 'm', 'x', 'y', 'z', 'vx', 'vy', 'vz' (nbody.py:71-115):

    a_x[j] = sum over i != j of G m_i (x_i - x_j) / max(r_ij, 1)^3        (y, z alike)
    vx += dt * a_x          then          x += dt * vx   with the NEW vx

The reference builds about ten n x n expressions per move.  method='fused' (the default) gloms the four (n,) arrays
'x', 'y', 'z', 'm' once per move (4 n elements) and runs ONE shuffle over the row bands of galaxy['x'] whose tile body
is one _nbody.nbody_accel per band (HipBackend: sp_nbody_accel -- every pair in registers, nothing of size n x n
allocated) into three (n,) targets.  method='expr' is the reference's expression, line for line, on the map and reduce
kernels, with the diagonal set element-wise (below); it is kept for comparison and for the benchmark.

Deviations from the reference:
  * What its `set_diagonal` computes as written is not kept.  Its mapper returns the bare scalar in place of a WHOLE
    tile whenever the tile's upper-left corner has row == column, and the (n,) against (n, 1) broadcast is cut into
    column bands, so only the first band ever qualifies.  Read as "the tile becomes the scalar", every force is zeroed
    with one worker (all accelerations are 0), and with four the first band's are 0 and the true diagonal of the
    other bands is 0 / 0 = NaN; in the reference itself the map operator asks the returned float for its shape and
    the move raises AttributeError (tests/golden/nbody_w4.npz records what the recording run saw as `as_written_vx`:
    NaN throughout).  Its docstrings state the intent -- "Set the force (acceleration) a body exerts on itself to
    zero" -- and that, the element-wise diagonal, is what both methods here compute: 'expr' adds eye(n) to r (so
    r_ii = 1 and f_ii = G m 0 / 1 = 0, which makes the second set_diagonal redundant), 'fused' adds +0 for i == j.
  * 'fused' divides once per pair, w = (G m_i) / ((r r) r), and multiplies the three components by w, where the
    reference divides G m dx by r**3 three times: a rounding or two per term (the tests' bound covers both).
  * The six arrays a move changes are evaluated at the end of the move.  The reference has that `eager` commented
    out, and its expression graph grows by a move's worth every move.
  * `move` takes `method`, `g` and `rmin` (the reference: G and 1.0), `simulate` takes `dt`; arrays may be float32
    (the move is then in float32), integer arrays are converted to float64; a bad method, an rmin that is not finite
    and > 0, a g that is not finite, arrays that are not 1-D and of equal length raise ValueError, a missing key
    KeyError, complex or object arrays TypeError."""
import numpy as np

from .. import expr
from ..array import distarray, extent
from . import _nbody

G = 6.67384e-11       # m^3 / (kg s^2)
dt = 60 * 60 * 24 * 365.25  # a year in seconds
r_ly = 9.4607e15      # a light year in m
m_sol = 1.9891e30     # a solar mass in kg

METHODS = ('fused', 'expr')
KEYS = ('m', 'x', 'y', 'z', 'vx', 'vy', 'vz')
_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def random_galaxy(n):
  """A galaxy of `n` bodies at rest, float64 as in the reference: masses of 1 to 1.1 solar masses in a cube of a
  hundredth of a light year.  These SI units overflow float32 -- r**3 is about 1e42 -- so a float32 run needs scaled
  units (lengths and masses of order 1) and its own `g`."""
  dtype = np.float64
  return {
      'm': (expr.rand(n) + dtype(10)) * dtype(m_sol / 10),
      'x': (expr.rand(n) - dtype(0.5)) * dtype(r_ly / 100),
      'y': (expr.rand(n) - dtype(0.5)) * dtype(r_ly / 100),
      'z': (expr.rand(n) - dtype(0.5)) * dtype(r_ly / 100),
      'vx': expr.zeros((n,), dtype=dtype),
      'vy': expr.zeros((n,), dtype=dtype),
      'vz': expr.zeros((n,), dtype=dtype),
  }


def _accel_mapper(array, ex, bodies=None, g=None, rmin=None, ax=None, ay=None, az=None):
  """Tile body of the shuffle: the accelerations of this band of bodies under all of them, into the three targets."""
  lo, hi = ex.ul[0], ex.lr[0]
  n = array.shape[0]
  if isinstance(array.fetch(ex), distarray.Absent):        # (a band of another rank)
    tiles = [distarray.Absent((hi - lo,), np.dtype(bodies[0].dtype))] * 3
  else:
    tiles = _nbody.nbody_accel(*bodies, lo, hi - lo, g=g, rmin=rmin)
  where = extent.create((lo,), (hi,), (n,))
  for target, tile in zip((ax, ay, az), tiles):
    target.update(where, tile)
  return []


_accel_mapper.yields_fresh_tensors = True      # the kernel's output (or NumPy's), never a fetched tile


def _accel_fused(x, y, z, m, n, dtype, g, rmin):
  bodies = [np.ascontiguousarray(np.asarray(a.glom()), dtype=dtype) for a in (x, y, z, m)]
  ax, ay, az = (expr.ndarray((n,), dtype=dtype, tile_hint=(n,)) for _ in range(3))
  expr.shuffle(x, _accel_mapper, kw={'bodies': bodies, 'g': g, 'rmin': rmin, 'ax': ax, 'ay': ay, 'az': az},
               shape_hint=(1,)).evaluate()
  return [ax, ay, az]


def _accel_expr(x, y, z, m, n, dtype, g, rmin):
  """The reference's expression (nbody.py:81-111); the comments name its lines."""
  x, y, z, m = (expr.lazify(a) for a in (x, y, z, m))
  minus, two, three = dtype.type(-1), dtype.type(2), dtype.type(3)   # (Python scalars would promote float32)
  dx = (x - expr.reshape(x, (n, 1))) * minus                  # dx = (galaxy['x'] - dx_new) * -1
  dy = (y - expr.reshape(y, (n, 1))) * minus
  dz = (z - expr.reshape(z, (n, 1))) * minus
  r = expr.sqrt(dx ** two + dy ** two + dz ** two)                # r = sqrt(dx**2 + dy**2 + dz**2)
  r = r + expr.eye(n, n, dtype=dtype)                         # r = set_diagonal(r, 1.0), element-wise
  r = expr.maximum(r, dtype.type(rmin))                       # mask = r < 1.0; r = r * ~mask + 1.0 * mask
  mc = expr.reshape(m, (n, 1))
  gt = dtype.type(g)
  # (the scalar on the right: on the left a NumPy scalar decides the product's type itself, and under a fused sum the
  #  float32 run came out as float64; the product's bits are the same)
  fx = mc * gt * dx / r ** three                                  # fx = G*m*dx / r**3  (f_ii = G m 0 / 1 = 0)
  fy = mc * gt * dy / r ** three
  fz = mc * gt * dz / r ** three
  return [expr.sum(f, axis=0) for f in (fx, fy, fz)]


def _prepare(galaxy, method, g, rmin):
  """(the seven arrays evaluated, n, dtype, g, rmin), or the refusals."""
  if method not in METHODS:
    raise ValueError('move: unknown method %r (%s)' % (method, ' '.join(METHODS)))
  arrays = {}
  for key in KEYS:
    a = galaxy[key]
    if not isinstance(a, np.ndarray):
      a = expr.evaluate(a)
    if np.dtype(a.dtype).kind not in 'fiub':
      raise TypeError("move: galaxy[%r] of dtype %s; the arrays are real numbers" % (key, np.dtype(a.dtype)))
    arrays[key] = expr.evaluate(expr.from_numpy(a)) if isinstance(a, np.ndarray) else a
  own = [np.dtype(a.dtype) for a in arrays.values()]
  dtype = own[0] if own[0] in _FLOATS and all(d == own[0] for d in own) else np.dtype(np.float64)
  for key in KEYS:
    if np.dtype(arrays[key].dtype) != dtype:
      arrays[key] = expr.astype(arrays[key], dtype)
  shapes = [tuple(arrays[key].shape) for key in KEYS]
  _, n, _, _, g, rmin, _ = _nbody.check_operands([dtype] * len(KEYS), shapes, 0, 0, g, rmin, what='move')
  return {key: expr.evaluate(a) for key, a in arrays.items()}, n, dtype, g, rmin


def move(galaxy, dt, method='fused', g=G, rmin=1.0):
  """Move the bodies: first the forces change the velocities, then the NEW velocities move the positions
  (nbody.py:71-115).  `galaxy` is changed in place: its six arrays 'vx' .. 'z' are replaced by evaluated distributed
  arrays ('m' only where it had to be converted).  method: 'fused' (one all-pairs kernel per band of bodies) or 'expr'
  (the reference's n x n expression); g: the gravitational constant in the galaxy's units; rmin: the distance below
  which two bodies attract as if they were rmin apart (the reference: 1.0).  See the module docstring for the
  deviations and the errors."""
  a, n, dtype, g, rmin = _prepare(galaxy, method, g, rmin)
  accel = (_accel_fused if method == 'fused' else _accel_expr)(a['x'], a['y'], a['z'], a['m'], n, dtype, g, rmin)
  step = dtype.type(dt)
  for v, acc in zip(('vx', 'vy', 'vz'), accel):                 # galaxy['vx'] += dt*expr.sum(fx, axis=0)
    galaxy[v] = (expr.lazify(a[v]) + step * expr.lazify(acc)).optimized().evaluate()
  for p, v in (('x', 'vx'), ('y', 'vy'), ('z', 'vz')):           # galaxy['x'] += dt*galaxy['vx']
    galaxy[p] = (expr.lazify(a[p]) + step * expr.lazify(galaxy[v])).optimized().evaluate()
  # (evaluated here: the reference's expr.eager at the end of move is commented out)
  galaxy['m'] = a['m']


def simulate(galaxy, timesteps, dt=dt, **kw):
  """`timesteps` moves of `dt` seconds each; **kw goes to `move`."""
  for _ in range(int(timesteps)):
    move(galaxy, dt, **kw)
