"""Inputs, oracle and error bound of the affinity / normalised-Laplacian kernels of spectral clustering
(sp_affinity_degree, sp_affinity_matrix, examples/_spectral.py).  Pure NumPy.

Oracle.  The formulas of include/spartan_hip_spectral.h in numpy.longdouble from the stored operands, with gamma rounded
to the operands' dtype T once, as the kernel takes it:  A_ij = measure(p_i, p_j),  D_i = sum_j A_ij,  s_i = 1 / sqrt(D_i)
(1 where D_i is 0),  L_ij = A_ij s_i s_j with L_ii = 1.

Bound (derived, not measured).  u = 2^-24 or 2^-53, gamma_t = t u / (1 - t u).  The (1 + eps) factors are composed, not
added, so second-order terms are carried and no safety factor is needed.
  d2     each term (x - y)^2 carries three roundings and the sum of d terms d - 1 more: d2^ = d2 (1 + theta_{d+2})
  'euclidean'   the square root halves that and adds its own rounding:       e_a = gamma_{d+2} / 2 + u
  'manhattan'   |x - y| carries one rounding, the sum d - 1 more:            e_a = gamma_{d+1}   (gamma_d would do)
  'rbf'  the argument t = g d2 takes one more rounding, 1 + e_t = (1 + gamma_{d+2}) (1 + u); a relative error e_t of the
         argument is an ABSOLUTE error of the exponent, exp(-t (1 + delta)) = a exp(-t delta), so the error of a is
         a (exp(|t| e_t) - 1), about a |t| e_t; on top come the 2 ulp = 4 u the project states and tests for EXP
         (tests/test_op_semantics_gpu.py ULP_BOUND):          1 + e_a = exp(|t| e_t) (1 + 4 u)
         per entry, with the entry's own t.  The bound is relative only where t is bounded: the cases keep |t| <= 50
         (`oracle` asserts it), so e_a <= about 50 e_t + 4 u.
  D      the terms are non-negative, so in ANY order of summation the sum of n computed terms is within gamma_{n-1} <=
         gamma_n of their exact sum:   1 + e_D = (1 + max_j e_a) (1 + gamma_n), per row
  s      sqrt of a perturbed D, rounded, and a division, rounded:   1 + e_s = (1 + u) / ((1 - u) sqrt(1 - e_D));
         to first order e_D / 2 + 2 u.  s = 1 exactly where the computed D is 0, which it is exactly when D is 0 (a
         sum of non-negative terms none of which rounds to 0 from a non-zero value at |t| <= 50)
  L      the product of the two scales, rounded, times a, rounded:   1 + e_L = (1 + e_a) (1 + e_s_i) (1 + e_s_j) (1 + u)^2;
         the diagonal is exactly 1.
The NumPy restatement (examples/_spectral.py) uses under half of the bounds of D and L at every listed shape in both
dtypes, and of A's too except for 'euclidean' and 'manhattan' at d = 2 and 3, where a_ij carries three to five roundings,
the bound counts exactly those and single pairs reach 0.86 of it (tests/test_spectral_cases_cpu.py prints the shares and says how NumPy's
own float32 exp is kept out of the comparison).

Cases.  Points uniform in [0, 1)^d, so d2 <= d and, with gamma = 1 and d <= 33, t <= 33; rows 0 and 1 are the same
point when there are at least two (an off-diagonal distance of exactly 0).
"""
import functools

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
LD = np.longdouble
METRICS = ('rbf', 'euclidean', 'manhattan')
T_MAX = 50.0
# (m, n, d, r0): rows r0 .. r0 + m - 1 of n points with d features, at the edges of the tiling that was built
# (include/spartan_hip_spectral.h): tiles of 64 x 64, four columns to a thread, features in chunks of 16; 449 is the
# smallest n whose ceil(n / 64) = 8 column blocks are cut into two ranges.  Nothing is larger than 300 x 600.
SHAPES = (
    (1, 1, 1, 0), (1, 5, 0, 3), (63, 63, 2, 0), (64, 64, 15, 0), (65, 65, 16, 0), (64, 130, 17, 64), (2, 129, 3, 127),
    (130, 130, 33, 0), (70, 300, 2, 200), (66, 449, 3, 383),
)


def gamma_(t, dtype):
  tu = t * U[np.dtype(dtype)]
  assert tu < 1
  return tu / (1 - tu)


@functools.lru_cache(maxsize=None)
def case(n, d, dtype, seed=0):
  """points [n, d] in `dtype`, read-only."""
  rng = np.random.RandomState(20151101 + 7919 * seed + 31 * n + d)
  p = rng.rand(n, d).astype(dtype)
  if n >= 2:
    p[1] = p[0]
  p.setflags(write=False)
  return p


def planted():
  """(P [60, 2] float64, truth [60]): the golden input of tests/golden/spectral_w4.npz -- three planted groups."""
  rng = np.random.RandomState(7)
  centres = np.array([[0, 0], [3, 0.3], [0.4, 3]], np.float64)
  truth = np.arange(60) % 3
  p = centres[truth] + 0.35 * rng.randn(60, 2)
  return p, truth


def oracle(y, metric, gamma=1.0):
  """dict(A [n, n], t [n, n], D [n], s [n], L [n, n]) in longdouble for the points y (gamma rounded to y's dtype)."""
  assert metric in METRICS
  g = LD(np.dtype(y.dtype).type(gamma))
  yl = np.asarray(y, LD)
  n = yl.shape[0]
  dist = np.zeros((n, n), LD)
  for f in range(yl.shape[1]):
    t = yl[:, f:f + 1] - yl[:, f][None, :]
    dist += np.abs(t) if metric == 'manhattan' else t * t
  t = np.zeros((n, n), LD)
  if metric == 'rbf':
    t = g * dist
    assert not t.size or float(np.abs(t).max()) <= T_MAX, 'the bound is relative only for |t| <= %g' % T_MAX
    a = np.exp(-t)
  else:
    a = np.sqrt(dist) if metric == 'euclidean' else dist
  deg = a.sum(axis=1)
  root = np.sqrt(deg)
  root[root == 0] = 1
  s = 1 / root
  lap = a * s[:, None] * s[None, :]
  lap[np.arange(n), np.arange(n)] = 1
  return dict(A=a, t=np.abs(t), D=deg, s=s, L=lap)


@functools.lru_cache(maxsize=None)
def oracle_of_case(n, d, dtype, metric, gamma=1.0, seed=0):
  return oracle(case(n, d, np.dtype(dtype), seed), metric, gamma)


def eps(want, d, metric, dtype):
  """dict(a [n, n], D [n], s [n], L [n, n]): the relative bounds of the module docstring for the oracle `want` of n
  points with d features."""
  dt = np.dtype(dtype)
  u = U[dt]
  n = want['A'].shape[0]
  if metric == 'rbf':
    e_t = (1 + gamma_(d + 2, dt)) * (1 + u) - 1
    e_a = np.exp(np.asarray(want['t'], np.float64) * e_t) * (1 + 4 * u) - 1
  elif metric == 'euclidean':
    e_a = np.full((n, n), gamma_(d + 2, dt) / 2 + u)
  else:
    e_a = np.full((n, n), gamma_(d + 1, dt))
  e_d = (1 + (e_a.max(axis=1) if n else np.zeros((0,)))) * (1 + gamma_(max(n, 1), dt)) - 1
  e_s = (1 + u) / ((1 - u) * np.sqrt(1 - e_d)) - 1
  e_l = (1 + e_a) * (1 + e_s[:, None]) * (1 + e_s[None, :]) * (1 + u) ** 2 - 1
  return dict(a=e_a, D=e_d, s=e_s, L=e_l)


def _ratio(err, limit):
  """max err / limit over the entries (0 / 0 counts as 0)."""
  err, limit = np.asarray(err, np.float64), np.asarray(limit, np.float64)
  if not err.size:
    return 0.0
  with np.errstate(all='ignore'):
    r = np.where(err == 0, 0.0, err / limit)
  return float(np.max(r))


def scale_of(deg):
  """s in the dtype of the computed degrees, as the driver forms it: sqrt, zeros to 1, 1.0 / ..."""
  s = np.sqrt(deg)
  s[s == 0] = 1
  return (1.0 / s).astype(deg.dtype)


def check(y, r0, m, metric, want, deg=None, a=None, lap=None, label=''):
  """The outputs for the rows r0 .. r0 + m - 1 of the points y -- degrees [m], plain affinities [m, n], normalised
  matrix [m, n], any of them -- against the oracle `want` of y and the bound of y's shape and dtype.  Prints the
  measured shares of the bound first.  Returns them."""
  dt = np.dtype(y.dtype)
  n, d = y.shape
  b = eps(want, d, metric, dt)
  rows = slice(r0, r0 + m)
  shares = {}
  if deg is not None:
    deg = np.asarray(deg)
    assert deg.dtype == dt and deg.shape == (m,), (deg.dtype, deg.shape)
    shares['D'] = _ratio(np.abs(np.asarray(deg, LD) - want['D'][rows]), b['D'][rows] * want['D'][rows])
  if a is not None:
    a = np.asarray(a)
    assert a.dtype == dt and a.shape == (m, n), (a.dtype, a.shape)
    shares['A'] = _ratio(np.abs(np.asarray(a, LD) - want['A'][rows]), b['a'][rows] * want['A'][rows])
  if lap is not None:
    lap = np.asarray(lap)
    assert lap.dtype == dt and lap.shape == (m, n), (lap.dtype, lap.shape)
    shares['L'] = _ratio(np.abs(np.asarray(lap, LD) - want['L'][rows]), b['L'][rows] * want['L'][rows])
  print('%s: shares of the bound %s (largest e_a %.3g, e_D %.3g, e_L %.3g)'
        % (label, ' '.join('%s %.3g' % kv for kv in sorted(shares.items())),
           b['a'].max() if b['a'].size else 0.0, b['D'].max() if n else 0.0, b['L'].max() if b['L'].size else 0.0))
  assert all(v <= 1.0 for v in shares.values()), (label, shares)
  if lap is not None and m:
    assert np.all(lap[np.arange(m), r0 + np.arange(m)] == 1), label           # the diagonal: exactly 1
  if a is not None and m:
    assert np.all(a[np.arange(m), r0 + np.arange(m)] == (1 if metric == 'rbf' else 0)), label
  return shares


def partition(labels):
  """The clustering as a set of sets of point indices: label numbers are free."""
  labels = np.asarray(labels).reshape(-1)
  return frozenset(frozenset(np.flatnonzero(labels == v).tolist()) for v in np.unique(labels))
