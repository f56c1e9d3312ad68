"""Inputs, oracle, recipe and error bound of the fuzzy k-means step (sp_fuzzy_step, examples/_fuzzy.py).  Pure NumPy.

Oracle.  The formulas of include/spartan_hip_fuzzy.h in numpy.longdouble from the stored operands, with m, the
exponent e = 1 / (m - 1) and 1e-10 rounded to the operands' dtype T as the kernel takes them.

Recipe.  The distance as the kernel forms it, in T: d2 = (((x_0 - c_0)^2) + (x_1 - c_1)^2) + ..., rounded after every
operation.  The label is the first arg-max of d2 (a NaN counts as the largest value): the one output whose bits the
contract fixes without reference to an order of summation.

Bound (derived, not measured).  u = 2^-24 or 2^-53, gamma_t = t u / (1 - t u).  Every sum of the step has non-negative
terms, so every bound is relative; the (1 + eps) factors are composed, not added, so second-order terms are carried.
  dist   each term (x - c)^2 carries three roundings and the sum of d terms d - 1 more: d2^ = d2 (1 + theta_{d+2}); the
         square root halves that and adds its own rounding:   eps_d = gamma_{d+2} / 2 + u
  p      m = 2: p = dist, eps_p = eps_d.  Otherwise pow of a perturbed argument, (dist (1 + eps_d))^e, and the 2 ulp =
         4 u the project states and tests for POW (tests/test_op_semantics_gpu.py ULP_BOUND):
         1 + eps_p = (1 + eps_d)^e (1 + 4 u)
  u_ij   z = sum_j p_ij in ANY order is within gamma_{k-1} <= gamma_k of the sum of the computed p (adding a zero is
         exact), the division rounds once:   1 + eps_u = (1 + eps_p) (1 + u) / ((1 - eps_p) (1 - gamma_k))
         (to first order 2 eps_p + gamma_k + u);   |u^ - u| <= eps_u u
  w      m = 2: 1 + eps_w = (1 + eps_u)^2 (1 + u); otherwise (1 + eps_u)^m (1 + 4 u)
  wsum   relative (1 + eps_w) (1 + gamma_n) - 1
  sums   |delta| <= ((1 + eps_w) (1 + gamma_{n+1}) - 1) sum_i w_ij |x_if|: n products, each rounded, n - 1 additions, in
         any order of rows
  label  the computed d2 are within gamma_{d+2} of the true ones, so the true membership at the returned label is at
         least (1 - 2 eps_u) times the row's largest; no row is left out.
The NumPy restatement of the step (examples/_fuzzy.step_numpy) uses under 10 % of this bound at (130, 70, 20, m = 2),
(65, 3, 257, 2), (200, 129, 5, 1.5), (100, 64, 33, 3) and (1000, 17, 64, 2) in both dtypes, and its labels equal the
oracle's (tests/test_fuzzy_cases_cpu.py prints the figures).

Two iterations (the driver's tests).  centers = sums / wsum per entry: with eS, eW the relative bounds of sums and wsum,
  |c^_jf - c_jf| <= ((1 + eS) (1 + u) / (1 - eW) - 1) a_jf,        a_jf = sum_i w_ij |x_if| / sum_i w_ij.
An iteration that starts from centres off by delta_j = ||c^_j - c_j||_2 sees every distance off by at most delta_j (the
triangle inequality), relatively by rho = max_ij delta_j / dist_ij; then p is off by (1 + rho)^e, u by
(1 + rho)^e / (1 - rho)^e =: 1 + eta_u (numerator and normaliser move apart at worst), w by (1 + eta_u)^m =: 1 + eta_w,
and sums and wsum, having non-negative terms, by the same factor on top of their own rounding:
  |c2^_jf - c2_jf| <= ((1 + eS) (1 + eta_w) (1 + u) / ((1 - eW) (1 - eta_w)) - 1) a_jf.
delta_j of the first iteration is the norm of its bound's row plus, in float32, the rounding u ||c_j|| of the centres
handed to the second.  The bound is void (and `two_step_bound` asserts) unless rho < 1e-2.

Cases.  Points and centres uniform in [0, 1) (no underflow in float32); centre 0 equals point 3 exactly (the 1e-10
path); the last centre is bit-identical to centre 1 (a tie, which goes to the lower index: the last centre is never a
label); a variant puts a NaN into row 5.
"""
import functools

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
LD = np.longdouble
MS = (2.0, 1.5, 3.0)


def gamma(t, dtype):
  tu = t * U[np.dtype(dtype)]
  assert tu < 1
  return tu / (1 - tu)


@functools.lru_cache(maxsize=None)
def case(n, k, d, dtype, seed=0, nan_row=False):
  """(points [n, d], centers [k, d]) in `dtype`, read-only."""
  rng = np.random.RandomState(20151019 + 7919 * seed + 31 * n + 17 * k + d)
  x = rng.rand(n, d).astype(dtype)
  c = rng.rand(k, d).astype(dtype)
  if n > 3:
    c[0] = x[3]
  if k >= 3:
    c[k - 1] = c[1]
  if nan_row:
    assert n > 5 and d > 0
    x[5, d // 2] = np.nan
  x.setflags(write=False)
  c.setflags(write=False)
  return x, c


def scalars(m, dtype):
  """(m, e, tiny) as the kernel takes them: each rounded to `dtype` once; and whether m == 2 exactly."""
  dt = np.dtype(dtype)
  return dt.type(m), dt.type(1.0 / (float(m) - 1.0)), dt.type(1e-10), float(m) == 2.0


def recipe_d2(x, c):
  """d2 [n, k] in the dtype of x and c, as the kernel forms it."""
  dt = x.dtype
  d2 = np.zeros((x.shape[0], c.shape[0]), dt)
  with np.errstate(all='ignore'):
    for f in range(x.shape[1]):
      t = x[:, f:f + 1] - c[:, f][None, :]
      d2 = d2 + t * t
  assert d2.dtype == dt
  return d2


def recipe_labels(x, c):
  return np.argmax(recipe_d2(x, c), axis=1).astype(np.int64) if x.shape[0] else np.zeros((0,), np.int64)


def oracle(x, c, m, dtype=None):
  """dict(u [n, k], z [n], labels [n], wsum [k], sums [k, d], abs_sums [k, d]) in longdouble; `dtype`: the type whose
  rounding of m, e and 1e-10 is used (default: that of x)."""
  mt, e, tiny, m2 = scalars(m, dtype if dtype is not None else x.dtype)
  xl, cl = np.asarray(x, LD), np.asarray(c, LD)
  n, k = xl.shape[0], cl.shape[0]
  with np.errstate(all='ignore'):
    d2 = np.zeros((n, k), LD)
    for f in range(xl.shape[1]):
      t = xl[:, f:f + 1] - cl[:, f][None, :]
      d2 += t * t
    dist = np.sqrt(d2)
    dist[dist == 0] = LD(tiny)
    p = dist if m2 else dist ** LD(e)
    z = p.sum(axis=1)
    u = p / z[:, None]
    w = u * u if m2 else u ** LD(mt)
    return dict(dist=dist, u=u, z=z, labels=np.argmax(u, axis=1) if n else np.zeros((0,), np.int64), w=w,
                wsum=w.sum(axis=0), sums=w.T.dot(xl), abs_sums=w.T.dot(np.abs(xl)))


@functools.lru_cache(maxsize=None)
def oracle_of_case(n, k, d, dtype, m, seed=0, nan_row=False):
  return oracle(*case(n, k, d, np.dtype(dtype), seed, nan_row), m=m)


def eps(n, k, d, m, dtype):
  """dict of the relative bounds of the module docstring for a step of n rows, k centres, d features."""
  dt = np.dtype(dtype)
  u = U[dt]
  _, e, _, m2 = scalars(m, dt)
  e, mt = float(e), float(dt.type(m))
  eps_d = gamma(d + 2, dt) / 2 + u
  eps_p = eps_d if m2 else (1 + eps_d) ** e * (1 + 4 * u) - 1
  eps_u = (1 + eps_p) * (1 + u) / ((1 - eps_p) * (1 - gamma(k, dt))) - 1
  eps_w = (1 + eps_u) ** 2 * (1 + u) - 1 if m2 else (1 + eps_u) ** mt * (1 + 4 * u) - 1
  return dict(d=eps_d, p=eps_p, u=eps_u, w=eps_w, wsum=(1 + eps_w) * (1 + gamma(max(n, 1), dt)) - 1,
              sums=(1 + eps_w) * (1 + gamma(n + 1, dt)) - 1)


def _ratio(err, limit):
  """max err / limit over the entries (0 / 0 counts as 0)."""
  err, limit = np.asarray(err, np.float64), np.asarray(limit, np.float64)
  if not err.size:
    return 0.0
  with np.errstate(all='ignore'):
    r = np.where(err == 0, 0.0, err / limit)
  return float(np.max(r))


def check_step(x, c, m, labels, sums, wsum, u=None, want=None, label=''):
  """Every output of a step on (x, c) against the oracle `want` (default: computed here) and the bound of the step's
  own shape and dtype; labels against the recipe, bit for bit.  Prints the measured shares of the bound first.  Returns
  the largest share."""
  dt = np.dtype(x.dtype)
  n, d = x.shape
  k = c.shape[0]
  if want is None:
    want = oracle(x, c, m)
  b = eps(n, k, d, m, dt)
  labels, sums, wsum = np.asarray(labels), np.asarray(sums), np.asarray(wsum)
  assert labels.dtype == np.int64 and labels.shape == (n,), (labels.dtype, labels.shape)
  assert sums.dtype == dt and sums.shape == (k, d) and wsum.dtype == dt and wsum.shape == (k,)
  shares = {}
  shares['wsum'] = _ratio(np.abs(np.asarray(wsum, LD) - want['wsum']), b['wsum'] * want['wsum'])
  shares['sums'] = _ratio(np.abs(np.asarray(sums, LD) - want['sums']), b['sums'] * want['abs_sums'])
  if u is not None:
    u = np.asarray(u)
    assert u.dtype == dt and u.shape == (n, k)
    shares['u'] = _ratio(np.abs(np.asarray(u, LD) - want['u']), b['u'] * want['u'])
  if n:
    at_label = want['u'][np.arange(n), labels]
    shares['label'] = _ratio(want['u'].max(axis=1) - at_label, 2 * b['u'] * want['u'].max(axis=1))
  exact = labels.tobytes() == recipe_labels(x, c).tobytes()
  print('%s: shares of the bound %s (eps_u %.3g, eps_sums %.3g); labels %s the recipe'
        % (label, ' '.join('%s %.3g' % kv for kv in sorted(shares.items())), b['u'], b['sums'],
           'equal' if exact else 'DIFFER FROM'))
  assert all(v <= 1.0 for v in shares.values()), (label, shares)
  assert exact, label
  if n:
    assert labels.min() >= 0 and labels.max() < k
  return max(shares.values()) if shares else 0.0


def centers_of(want):
  with np.errstate(all='ignore'):
    return want['sums'] / want['wsum'][:, None]


def two_step_bound(x, c0, m, dtype):
  """(c1, b1, c2, b2): the exact centres after one and two iterations from c0 (longdouble) and the per-entry bounds on
  what a run in `dtype` computes, as the module docstring derives them."""
  dt = np.dtype(dtype)
  u = U[dt]
  n, d = x.shape
  k = c0.shape[0]
  b = eps(n, k, d, m, dt)
  _, e, _, _ = scalars(m, dt)
  e, mt = float(e), float(dt.type(m))
  w1 = oracle(np.asarray(x, dt), np.asarray(c0, dt), m, dtype=dt)
  c1 = centers_of(w1)
  a1 = w1['abs_sums'] / w1['wsum'][:, None]
  b1 = ((1 + b['sums']) * (1 + u) / (1 - b['wsum']) - 1) * a1
  w2 = oracle(np.asarray(x, dt), c1, m, dtype=dt)
  c2 = centers_of(w2)
  a2 = w2['abs_sums'] / w2['wsum'][:, None]
  delta = np.sqrt((b1 ** 2).sum(axis=1))
  if dt != np.dtype(np.float64):
    delta = delta + u * np.sqrt((c1 ** 2).sum(axis=1))
  rho = float((delta[None, :] / w2['dist']).max())
  assert rho < 1e-2, 'the bound is void: rho = %g' % rho
  eta_u = (1 + rho) ** e / (1 - rho) ** e - 1
  eta_w = (1 + eta_u) ** mt - 1
  b2 = ((1 + b['sums']) * (1 + eta_w) * (1 + u) / ((1 - b['wsum']) * (1 - eta_w)) - 1) * a2
  return c1, b1, c2, b2
