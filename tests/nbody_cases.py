"""Cases, oracle and derived bounds of the all-pairs gravity kernel (sp_nbody_accel, include/spartan_hip_nbody.h) and of
the n-body driver (spartan_amd/examples/nbody.py).  Shared by the CPU and the GPU tests; nothing here touches a device.

THE BOUND OF AN ACCELERATION.  u = eps / 2 is the unit roundoff of the arrays' dtype T.  For target j and source i,
every operation rounded once (relative error <= u), to first order in u:
    dx = x_i - x_j                          u
    q  = (dx dx + dy dy) + dz dz            dx dx: 2 u + u = 3 u; all three summands are >= 0, so the two additions
                                            keep the largest relative error and add u each: 5 u
    r  = sqrt(q)                            5 u / 2 + u = 3.5 u     (IEEE square root)
    r3 = (r r) r                            r r: 7 u + u = 8 u;  (r r) r: 8 u + 3.5 u + u = 12.5 u
    w  = (T(g) m_i) / r3                    T(g) m_i: u (T(g) and T(rmin) are the problem's constants: the oracle
                                            takes them as rounded);  the division: u + 12.5 u + u = 14.5 u
    t  = w dx                               14.5 u + u (dx) + u = 16.5 u
    where r is clamped it is T(rmin) exactly and the term's error is smaller (4.5 u)
The n - 1 terms of a target (the zeros of i == j and of the padding are added exactly) are then added in SOME order:
a term passes through at most n - 2 additions that round, (n - 2) u.  Together |a_j - exact| <= c u sum_i |t_ij| with
c = n + 14.5.  The reference's own arithmetic, G*m*dx / r**3, gives G m: u, (G m) dx: 3 u, r**3 by pow: 3 * 3.5 u plus
pow's own error of up to an ulp (2 u) = 12.5 u, the division: 16.5 u -- the same.  The bound is stated with c = n + 17
(2.5 u of room for a pow that is an ulp worse than that), and gamma = c u / (1 - c u) takes care of the higher orders.
The clamp is a kink: a pair whose distance is within rounding of rmin may be clamped in T and not in the oracle (or
the other way round), which changes r3 by at most the same 12.5 u -- but to keep that case out of every check, the
builders assert that no pair is within relative 1e-3 of rmin, except the pairs placed deliberately at exactly
rmin / 2 and exactly coincident.

THE BOUND OF A TRAJECTORY (first order).  A move is  v' = fl(v + fl(T(dt) a)),  x' = fl(x + fl(T(dt) v')).  With
E_x[i], E_v[i] the error bounds so far (per body, the largest over the components):
    E_a[j] = gamma S_j                                   (the bound above, S_j = sum_i |t_ij| per component)
             + sum_i 6.2 g m_i / max(r_ij, rmin)^3 (E_x[i] + E_x[j])
      the sensitivity of a term to the positions: |d t_c / d dx_k| <= g m / r^3 (delta_ck + 3 |dx_c| |dx_k| / r^2), and
      summed over k that is at most (1 + 3 sqrt(3)) g m / r^3 < 6.2 g m / r^3; every dx_k is off by at most E_x[i] + E_x[j]
    E_v' = E_v + dt E_a + 3 u |dt a| + u |v'|            (T(dt), the product and the sum round once each)
    E_x' = E_x + dt E_v' + 3 u |dt v'| + u |x'|
evaluated along the oracle's trajectory in longdouble."""
import functools

import numpy as np

LD = np.longdouble
BLOCK, CLASSES, WORKGROUPS = 64, 4, 1024      # SP_NBODY_BLOCK, SP_NBODY_WAVES, SP_NBODY_WORKGROUPS
UNIT_G, UNIT_RMIN = 1.0, 0.05
NEAR = 1e-3                                   # no pair within this relative distance of rmin

G = 6.67384e-11
YEAR = 60 * 60 * 24 * 365.25
R_LY = 9.4607e15
M_SOL = 1.9891e30


def unit_roundoff(dtype):
  return float(np.finfo(np.dtype(dtype)).eps) / 2


def gamma(n, dtype):
  c = (n + 17) * unit_roundoff(dtype)
  return c / (1 - c)


def _distances(x, y, z):
  d = [np.asarray(v, LD)[:, None] - np.asarray(v, LD)[None, :] for v in (x, y, z)]
  return np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])


def _near_rmin(x, y, z, rmin, placed=()):
  """[n, n] bool: the pairs within relative NEAR of rmin, the `placed` pairs (i, j) left out."""
  near = np.abs(_distances(x, y, z) - LD(rmin)) <= NEAR * rmin
  for i, j in placed:
    near[i, j] = near[j, i] = False
  return near


def assert_clear_of_rmin(x, y, z, rmin, placed=()):
  """The cap: no pair within relative NEAR of rmin, except the `placed` pairs."""
  near = _near_rmin(x, y, z, rmin, placed)
  assert not near.any(), np.argwhere(near)[:4]


def placed_pairs(n):
  return (1, n - 2), (3, n // 2 + 1)


@functools.lru_cache(maxsize=None)
def _unit_case(n, dtype, seed, kind):
  dt = np.dtype(dtype)
  assert kind in ('random', 'placed')
  for attempt in range(64):                 # (the first draw that keeps the cap; which one depends on the arguments only)
    rng = np.random.default_rng(1000 * n + seed + 7919 * attempt)
    x, y, z = (rng.uniform(0.0, 1.0, n).astype(dt) for _ in range(3))
    mass = rng.uniform(0.5, 1.5, n).astype(dt)
    placed = []
    if kind == 'placed':
      assert n >= 8
      (a, b), (c, d) = placed = placed_pairs(n)
      x[b], y[b], z[b] = x[a] + dt.type(UNIT_RMIN) / 2, y[a], z[a]        # a pair at rmin / 2 (within rounding of x)
      x[d], y[d], z[d] = x[c], y[c], z[c]                                  # a pair exactly coincident
    if not _near_rmin(x, y, z, dt.type(UNIT_RMIN), placed).any():
      break
  assert_clear_of_rmin(x, y, z, dt.type(UNIT_RMIN), placed)
  for v in (x, y, z, mass):
    v.setflags(write=False)
  return x, y, z, mass, tuple(placed)


def unit_case(n, dtype, seed=0, kind='random'):
  """(x, y, z, mass) in `dtype`, read-only: positions in the unit cube, masses 0.5 .. 1.5; run with g = UNIT_G and
  rmin = UNIT_RMIN.  kind 'placed': bodies 1 and n - 2 are rmin / 2 apart, bodies 3 and n // 2 + 1 coincide."""
  return _unit_case(int(n), np.dtype(dtype).name, int(seed), kind)[:4]


@functools.lru_cache(maxsize=None)
def golden_input():
  """The galaxy tests/golden/nbody_w4.npz is recorded on: 24 bodies from a seeded generator by random_galaxy's
  formulas (SI units), float64, at rest; the dict of seven read-only arrays."""
  rng = np.random.default_rng(20261020)
  n = 24
  galaxy = {'m': (rng.random(n) + 10.0) * (M_SOL / 10)}
  for key in ('x', 'y', 'z'):
    galaxy[key] = (rng.random(n) - 0.5) * (R_LY / 100)
  for key in ('vx', 'vy', 'vz'):
    galaxy[key] = np.zeros(n)
  for v in galaxy.values():
    assert v.dtype == np.float64
    v.setflags(write=False)
  return galaxy


def oracle(x, y, z, mass, g, rmin, targets=None):
  """(a [3, m], S [3, m]) in longdouble for the targets (default: all): the exact sums of the terms of the inputs as
  given (g and rmin rounded to the arrays' dtype first, as the kernel takes them), and S = sum_i |t_ij|."""
  dt = np.asarray(x).dtype
  with np.errstate(all='ignore'):
    gt, rt = LD(dt.type(g)), LD(dt.type(rmin))
  xs, ys, zs, ms = (np.asarray(v, LD) for v in (x, y, z, mass))
  n = xs.shape[0]
  targets = np.arange(n) if targets is None else np.asarray(targets)
  a, s = np.zeros((3, len(targets)), LD), np.zeros((3, len(targets)), LD)
  with np.errstate(all='ignore'):
    for c, j in enumerate(targets):
      dx, dy, dz = xs - xs[j], ys - ys[j], zs - zs[j]
      r = np.sqrt(dx * dx + dy * dy + dz * dz)
      r = np.where(r < rt, rt, r)
      w = gt * ms / (r * r * r)
      w[j] = 0
      for k, d in enumerate((dx, dy, dz)):
        t = w * d
        t[j] = 0
        a[k, c], s[k, c] = t.sum(), np.abs(t).sum()
  return a, s


def share(err, bound):
  """max err / bound over the entries (0 / 0 counts as 0; anything over a bound of 0 as inf)."""
  err, bound = np.asarray(err, LD), np.asarray(bound, LD)
  with np.errstate(all='ignore'):
    q = np.where(err == 0, 0, err / bound)
  return float(np.max(q)) if q.size else 0.0


def check_accel(got, x, y, z, mass, g, rmin, label, targets=None, want=None):
  """Every entry of got = (ax, ay, az) within gamma S of the oracle; prints the measured share first."""
  n, dt = len(x), np.asarray(x).dtype
  a, s = oracle(x, y, z, mass, g, rmin, targets) if want is None else want
  got = np.asarray([np.asarray(v) for v in got])
  assert got.dtype == dt and got.shape == a.shape, (got.dtype, got.shape, a.shape)
  assert np.isfinite(got).all(), label
  sh = share(np.abs(np.asarray(got, LD) - a), gamma(n, dt) * s)
  print('%s: |a - exact| is %.3g of gamma * sum|t| (gamma = %.3g)' % (label, sh, gamma(n, dt)))
  assert sh <= 1.0, label
  return sh


def ranges_of(n, splits):
  """The number of source ranges (nbody_ranges of csrc/nbody.hip): from n and splits alone."""
  nb = -(-n // BLOCK)
  if nb <= 1:
    return 1
  if splits >= 1:
    return min(splits, nb)
  return min(-(-WORKGROUPS // nb), nb)


def range_sum(terms, lo, hi):
  """The header's levels 1 and 2 for the sources lo .. hi - 1 (hi - lo a multiple of 64, `terms` zero-padded): class c
  takes the terms with i mod 4 == c in ascending order onto +0; the four are combined as (p0 + p1) + (p2 + p3)."""
  dt = terms.dtype
  p = []
  with np.errstate(all='ignore'):
    for c in range(CLASSES):
      acc = dt.type(0)
      for v in terms[lo + c:hi:CLASSES]:
        acc = acc + v
      p.append(acc)
    return (p[0] + p[1]) + (p[2] + p[3])


def ordered_sum(terms, n, splits=0):
  """The sum of one target's [n] terms in the order include/spartan_hip_nbody.h states, in the terms' dtype."""
  dt = terms.dtype
  nb = -(-n // BLOCK)
  padded = np.zeros(nb * BLOCK, dt)
  padded[:n] = terms
  ranges = ranges_of(n, splits)
  cuts = [(g * nb // ranges) * BLOCK for g in range(ranges + 1)]
  parts = [range_sum(padded, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
  acc = parts[0]
  with np.errstate(all='ignore'):
    for p in parts[1:]:
      acc = acc + p
  assert acc.dtype == dt
  return acc


def ordered_accel(x, y, z, mass, g, rmin, splits=0, targets=None):
  """(ax, ay, az): ordered_sum of examples/_nbody.pair_terms for every target -- what the kernel must give bit for bit."""
  from spartan_amd.examples import _nbody
  n = len(x)
  targets = range(n) if targets is None else targets
  out = [[], [], []]
  for j in targets:
    for o, t in zip(out, _nbody.pair_terms(x, y, z, mass, j, g, rmin)):
      o.append(ordered_sum(t, n, splits))
  return tuple(np.asarray(o, np.asarray(x).dtype) for o in out)


def trajectory(galaxy, steps, step, g, rmin, dtype):
  """The oracle's trajectory and its first-order error bound for a run in `dtype`: a list, entry s = the state after s
  moves, each (state, bound) with state = {'x': .., 'vx': .., ..} in longdouble and bound = {'x': E_x [n], 'v': E_v [n]}
  (per body, for every component).  Entry 0 is the start (bounds 0); entry s >= 1 also has state['a'] = the [3, n]
  accelerations that move used and bound['a'] = their [3, n] bound gamma S + the sensitivity term."""
  dt = np.dtype(dtype)
  u = LD(unit_roundoff(dt))
  n = len(galaxy['m'])
  with np.errstate(all='ignore'):
    gt, rt, h = LD(dt.type(g)), LD(dt.type(rmin)), LD(dt.type(step))
  cur = {k: np.asarray(np.asarray(v, dt), LD) for k, v in galaxy.items()}
  mass = cur['m']
  ex, ev = np.zeros(n, LD), np.zeros(n, LD)
  out = [({k: v.copy() for k, v in cur.items()}, {'x': ex.copy(), 'v': ev.copy()})]
  for _ in range(steps):
    a, s = oracle(cur['x'], cur['y'], cur['z'], mass, gt, rt)
    r = np.maximum(_distances(cur['x'], cur['y'], cur['z']), rt)
    k = LD(6.2) * gt * mass[:, None] / (r * r * r)                       # [source i, target j]
    np.fill_diagonal(k, 0)
    sens = (k * (ex[:, None] + ex[None, :])).sum(axis=0)
    ea = gamma(n, dt) * s + sens[None, :]
    new = dict(cur)
    for c, (p, v) in enumerate((('x', 'vx'), ('y', 'vy'), ('z', 'vz'))):
      new[v] = cur[v] + h * a[c]
      new[p] = cur[p] + h * new[v]
    ev_c = [ev + h * ea[c] + 3 * u * np.abs(h * a[c]) + u * np.abs(new[v]) for c, v in enumerate(('vx', 'vy', 'vz'))]
    ev = np.max(ev_c, axis=0)
    ex_c = [ex + h * ev + 3 * u * np.abs(h * new[v]) + u * np.abs(new[p]) for p, v in (('x', 'vx'), ('y', 'vy'), ('z', 'vz'))]
    ex = np.max(ex_c, axis=0)
    cur = new
    state = {k: v.copy() for k, v in cur.items()}
    state['a'] = a
    out.append((state, {'x': ex.copy(), 'v': ev.copy(), 'a': ea}))
  return out


def min_separation(state):
  r = _distances(state['x'], state['y'], state['z'])
  np.fill_diagonal(r, np.inf)
  return float(r.min())
