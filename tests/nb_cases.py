"""Inputs, oracle and error bounds of the naive Bayes step (sp_nb_step, examples/_nb.py) and of the fit built on it
(examples/naive_bayes.py).  Pure NumPy.

Oracle.  The formulas of include/spartan_hip_nb.h in numpy.longdouble from the stored operands:
q_i = sum_j x_ij^2, r_i = sqrt(q_i / d), z_ij = x_ij / r_i, S_lj = the sum of z_ij over the rows of label l, df_j = the
rows with x_ij > 0, bad = 0 or 1 + the lowest row with a label outside 0 .. label_size - 1 (left out of S).  For the
fit: idf_j = log(n / (df_j + 1)) + 1, W = S idf, wl_l = sum_j W_lj, scores = log((W + alpha) / (wl + alpha d)).

Bound of the step (derived, not measured).  u = 2^-24 or 2^-53, gamma_t = t u / (1 - t u).  The (1 + eps) factors are
composed, not added, so second-order terms are carried and no safety factor is needed.
  q    d non-negative terms, each a rounded product, added in ANY order (a tree of d leaves has at most d - 1 additions
       on a path, and adding an exact 0 rounds nothing):                       1 + e_q = 1 + gamma_d
  r    the division by d (T(d) is exact below 2^24), the square root of that, and the root's own rounding:
       above  sqrt((1 + e_q) (1 + u)) (1 + u),  below  sqrt((1 - d u) (1 - u)) (1 - u);  e_r is the larger deviation
  z    a division by the computed r, rounded:                                  1 + e_z = (1 + u) / (1 - e_r)
       (below: (1 - u) / (1 + e_r) >= 1 - e_z)
  S    n_l computed terms in any order of summation (one range or several, one tile or several):
       |S^ - S| <= ((1 + e_z) (1 + gamma_{n_l - 1}) - 1) sum_{i in l} |z_ij|
  df and bad are exact.  A row whose r is 0 or NaN makes its label's row of S NaN, in the oracle as in the kernel: the
  NaN patterns must be identical and those entries have no bound.  Overflow and underflow are outside the bound: the
  cases keep the entries between 2^-6 and 2^4 or exactly 0.
Bound of the fit, stated for non-negative data and alpha > 0 (W + alpha >= alpha then: nothing cancels).  LOG carries
the 2 ulp = 4 u the project states and tests (tests/test_op_semantics_gpu.py ULP_BOUND); division is
IEEE.  E_* are absolute:
  idf  t = n / (df + 1) rounded once, log(t (1 + delta)) = log t + log(1 + delta):
       E_log = 4 u |log t| + (1 + 4 u) (-log(1 - u)),   E_idf = E_log + u (|idf| + E_log)
  W    'after' (this project: the summed S times idf, rounded):   E_W = (A + E_S) (idf + E_idf) (1 + u) - A idf
       'inside' (the reference: every z_ij times idf_j, rounded, then summed):
                                             E_W = A ((1 + e_z) (1 + u) (1 + gamma_{n_l - 1}) (idf + E_idf)) - A idf
       with A_lj = sum_{i in l} |z_ij| (= S for non-negative data)
  wl   d terms in any order:   E_wl = sum_j E_W + gamma_{d - 1} sum_j (W + E_W)
  num  W + T(alpha), den = wl + T(alpha d), each constant rounded once and each sum rounded:
       E_num = (E_W + alpha u) (1 + u) + u num,   E_den = (E_wl + alpha d u) (1 + u) + u den
  rho  = num / den rounded:   1 + e_rho = (1 + E_num / num) (1 + u) / (1 - E_den / den)
  scores   E = 4 u |log rho| + (1 + 4 u) (-log(1 - e_rho))
A comparison with the reference's recorded float64 outputs allows bound(T, 'after') + bound(float64, 'inside'): our
error against the exact value plus the reference's own.
The NumPy restatement (examples/_nb.py) stays under the step's bound at every listed shape in both dtypes
(tests/test_nb_cases_cpu.py prints the shares), so the bound is not one only the kernel's luck meets.

Cases.  Entries k / 64 with k in 1 .. 1023 (exact in float32), about a third of them 0; never a whole row of zeros
unless a test plants one.  Shapes at the edges of the tiling that was built (include/spartan_hip_nb.h): blocks of 64
rows, batches of 4 rows behind a ring of 8 to 48 rows in flight, lane sums over columns 64 apart, panels of 64, 128 or 256 columns depending on label_size, d
and the dtype.  Under splits = 0 the rows are cut into two ranges only from 961 rows on (16 blocks), so the tests force
splits = 2 and 3.
"""
import functools

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
LD = np.longdouble
LOG_ULP = 2.0            # tests/test_op_semantics_gpu.py ULP_BOUND
# (m, d, label_size, kind of labels)
SHAPES = (
    (1, 1, 1, 'random'), (8, 3, 2, 'random'), (9, 64, 128, 'random'), (63, 3, 2, 'random'), (64, 63, 5, 'equal'),
    (65, 64, 64, 'random'), (130, 65, 128, 'random'), (130, 130, 5, 'last'), (65, 257, 2, 'random'),
    (130, 257, 128, 'last'), (63, 130, 64, 'equal'), (200, 70, 5, 'random'), (600, 300, 5, 'random'),
)
SPLIT_SHAPES = ((130, 65, 128, 'random'), (200, 70, 5, 'random'), (600, 300, 5, 'random'))


def gamma_(t, dtype):
  tu = t * U[np.dtype(dtype)]
  assert np.all(tu < 1)
  return tu / (1 - tu)


@functools.lru_cache(maxsize=None)
def case(m, d, label_size, kind, dtype, seed=0):
  """(x [m, d] in `dtype`, labels int64 [m]), read-only."""
  rng = np.random.RandomState(20151120 + 7919 * seed + 131 * m + 17 * d + label_size)
  x = rng.randint(1, 1024, size=(m, d)) / 64.0
  x[rng.rand(m, d) < 1.0 / 3] = 0
  if d:
    x[np.arange(m), rng.randint(0, d, size=m)] = 1.0          # no row of zeros
  x = x.astype(dtype)
  if kind == 'random':
    labels = rng.randint(0, label_size, size=m)
  elif kind == 'equal':
    labels = np.full(m, label_size - 1)
  else:
    assert kind == 'last' and label_size >= 2
    labels = rng.randint(0, label_size - 1, size=m)
    labels[-1] = label_size - 1
  labels = labels.astype(np.int64)
  x.setflags(write=False)
  labels.setflags(write=False)
  return x, labels


def golden_input():
  """(data [120, 24] float64 counts, labels int64 [120], label_size 4, queries [10, 24]): the input of
  tests/golden/nb_w4.npz.  Four bands of 30 rows, no row of zeros, every label in every band."""
  rng = np.random.RandomState(20151122)
  n, d, label_size = 120, 24, 4
  labels = np.tile(np.arange(label_size), n // label_size)
  for b in range(4):
    rng.shuffle(labels[b * 30:(b + 1) * 30])
  # each label prefers its own six terms, so that a query has a clear best label
  rate = np.full((label_size, d), 0.6)
  for l in range(label_size):
    rate[l, l * 6:(l + 1) * 6] = 3.0
  data = rng.poisson(rate[labels]).astype(np.float64)
  data[np.arange(n), rng.randint(0, d, size=n)] += 1
  queries = rng.poisson(rate[np.arange(10) % label_size]).astype(np.float64)
  return data, labels.astype(np.int64), label_size, queries


def oracle(x, labels, label_size):
  """dict(S, A [label_size, d], count [label_size], z [m, d], df int64 [d], bad int64 [1]) in longdouble."""
  xl = np.asarray(x, LD)
  m, d = xl.shape
  labels = np.asarray(labels).reshape(m)
  with np.errstate(all='ignore'):
    q = (xl * xl).sum(axis=1)
    r = np.sqrt(q / LD(d))
    z = xl / r[:, None]
  ok = (labels >= 0) & (labels < label_size)
  s, a = np.zeros((label_size, d), LD), np.zeros((label_size, d), LD)
  count = np.zeros((label_size,), np.int64)
  for l in range(label_size):
    rows = ok & (labels == l)
    s[l], a[l], count[l] = z[rows].sum(axis=0), np.abs(z[rows]).sum(axis=0), rows.sum()
  wrong = np.flatnonzero(~ok)
  return dict(S=s, A=a, count=count, z=z, df=(np.asarray(x) > 0).sum(axis=0, dtype=np.int64).reshape(d),
              bad=np.array([wrong[0] + 1 if wrong.size else 0], np.int64))


@functools.lru_cache(maxsize=None)
def oracle_of_case(m, d, label_size, kind, dtype, seed=0):
  return oracle(*case(m, d, label_size, kind, np.dtype(dtype), seed), label_size)


def eps_z(d, dtype):
  """e_z of the module docstring for rows of d features."""
  dt = np.dtype(dtype)
  u = U[dt]
  assert d * u < 1
  above = np.sqrt((1 + gamma_(d, dt)) * (1 + u)) * (1 + u) - 1
  below = 1 - np.sqrt((1 - d * u) * (1 - u)) * (1 - u)
  e_r = max(above, below)
  return (1 + u) / (1 - e_r) - 1


def step_bound(want, d, dtype):
  """[label_size, d]: what |S^ - S| may be, absolute, for the oracle `want` (NaN where S is)."""
  dt = np.dtype(dtype)
  g = gamma_(np.maximum(want['count'] - 1, 0).astype(np.float64), dt)
  return ((1 + eps_z(d, dt)) * (1 + g)[:, None] - 1) * np.asarray(want['A'], np.float64)


def _ratio(err, limit):
  """max err / limit over the entries that are numbers (0 / 0 counts as 0)."""
  err, limit = np.asarray(err, np.float64), np.asarray(limit, np.float64)
  keep = ~np.isnan(limit)
  if not err.size or not keep.any():
    return 0.0
  with np.errstate(all='ignore'):
    r = np.where(err[keep] == 0, 0.0, err[keep] / limit[keep])
  return float(np.max(r))


def check_step(x, labels, label_size, s, df, bad, want=None, label=''):
  """The three outputs of a step on (x, labels) against the oracle and the bound of x's shape and dtype.  Prints the
  measured share of the bound first.  Returns it."""
  dt = np.dtype(x.dtype)
  m, d = x.shape
  want = oracle(x, labels, label_size) if want is None else want
  s, df, bad = np.asarray(s), np.asarray(df), np.asarray(bad)
  assert s.dtype == dt and s.shape == (label_size, d), (label, s.dtype, s.shape)
  assert df.dtype == np.int64 and df.shape == (d,) and bad.dtype == np.int64 and bad.shape == (1,), label
  b = step_bound(want, d, dt)
  with np.errstate(all='ignore'):
    share = _ratio(np.abs(np.asarray(s, LD) - want['S']), b)
  print('%s: |S - oracle| is %.3g of the bound (e_z %.3g, largest bound %.3g)'
        % (label, share, eps_z(d, dt) if d else 0.0, np.nanmax(b) if b.size and not np.isnan(b).all() else 0.0))
  assert np.array_equal(df, want['df']), label
  assert np.array_equal(bad, want['bad']), (label, bad, want['bad'])
  assert np.array_equal(np.isnan(s), np.isnan(np.asarray(want['S'], np.float64))), label
  assert share <= 1.0, (label, share)
  return share


def row_order_sum(z, labels, label_size):
  """The rows z_i. added onto zeros in row order, label by label, in z's dtype: what one range must give bit for bit."""
  s = np.zeros((label_size, z.shape[1]), z.dtype)
  with np.errstate(all='ignore'):
    for i, l in enumerate(np.asarray(labels).reshape(-1)):
      if 0 <= l < label_size:
        s[l] = s[l] + z[i]
  return s


def fit_oracle(x, labels, label_size, alpha):
  """dict(df, idf, W, wl, scores, and the step's oracle) of the whole fit in longdouble."""
  want = oracle(x, labels, label_size)
  n, d = x.shape
  idf = np.log(LD(n) / (np.asarray(want['df'], LD) + 1)) + 1
  w = want['S'] * idf[None, :]
  wl = w.sum(axis=1)
  with np.errstate(all='ignore'):
    scores = np.log((w + LD(alpha)) / (wl[:, None] + LD(alpha) * d))
  want.update(idf=idf, W=w, wl=wl, scores=scores)
  return want


def fit_bound(want, shape, alpha, dtype, order='after'):
  """dict(W, wl, scores): the absolute bounds of the module docstring for the fit oracle `want` of data of `shape`;
  order: 'after' (idf times the summed S) or 'inside' (the reference: idf inside the sum)."""
  assert order in ('after', 'inside') and alpha > 0
  dt = np.dtype(dtype)
  u = U[dt]
  c = 2 * LOG_ULP * u
  n, d = shape
  f = lambda v: np.asarray(v, np.float64)   # noqa: E731
  a, idf, w, wl = f(want['A']), f(want['idf']), f(want['W']), f(want['wl'])
  assert np.all(a == f(want['S'])) and np.all(a >= 0), 'the bound is stated for non-negative data'
  step = -np.log1p(-u)
  e_log = c * np.abs(idf - 1) + (1 + c) * step
  e_idf = e_log + u * (np.abs(idf) + e_log)
  e_z = eps_z(d, dt)
  g = gamma_(np.maximum(want['count'] - 1, 0).astype(np.float64), dt)[:, None]
  if order == 'after':
    e_s = ((1 + e_z) * (1 + g) - 1) * a
    e_w = (a + e_s) * (idf + e_idf)[None, :] * (1 + u) - a * idf[None, :]
  else:
    e_w = a * ((1 + e_z) * (1 + u) * (1 + g) * (idf + e_idf)[None, :]) - a * idf[None, :]
  e_wl = e_w.sum(axis=1) + gamma_(max(d - 1, 0), dt) * (w + e_w).sum(axis=1)
  num, den = w + alpha, wl + alpha * d
  e_num = (e_w + alpha * u) * (1 + u) + u * num
  e_den = (e_wl + alpha * d * u) * (1 + u) + u * den
  e_rho = (1 + e_num / num) * (1 + u) / (1 - (e_den / den)[:, None]) - 1
  e_scores = c * np.abs(f(want['scores'])) + (1 + c) * -np.log1p(-e_rho)
  return dict(W=e_w, wl=e_wl, scores=e_scores)
