"""Cases, the restated order and the yardstick for sp_svm_dca (include/spartan_hip_svm.h), examples/_svm.py and the
DisDCA driver.  No GPU, no backend: NumPy only.

  restated(...)    one pass in the header's stated order, scalar by scalar in the arrays' dtype T: the lane sums in
                   ascending order, the balanced tree, one rounding per operation.  Written apart from
                   examples/_svm.dca_numpy (which is vectorised) so that the two check each other; the kernel is held
                   to it byte for byte.
  yardstick(...)   the same recurrence in numpy.longdouble with plain sums (for float32: on the float32-rounded
                   inputs, which are exact in longdouble).
  run(body, ...)   a whole fit -- T iterations over the row bands, then w = sum(data * alpha * 1.0 / la / n, axis=0) --
                   with `body` as the pass.

The accuracy rule.  tests/golden/disdca_svm_w4.npz holds the reference's own run (alpha after iterations 1 and 3, w
after 3).  e_ref is the largest absolute distance of a recorded array to the yardstick's; a run of ours must lie within
8 e_ref of the yardstick in float64 and within 8 e_ref 2^29 in float32 (2^29: the ratio of the unit roundoffs).  Both
runs are the same recurrence and differ only in the order of 7-term sums; emulated at four shapes the ratio lay between
0.4 and 3.0, and the factor 8 covers that spread once more.  What the golden gives (max abs distance to the yardstick
over e_ref, and over 2^29 more in float32; the tests print every ratio before they assert; e_ref = 2.5e-16, 5.7e-16 and
8.4e-17 for alpha_1, alpha_3 and w_3):
                                                   alpha_1   alpha_3   w_3
    float64  restated = dca_numpy, driver 1 worker   1.12      0.73      1.49
             NumpyBackend driver, 4 workers          1.12      1.15      1.97
             HIP driver, 1 / 4 workers               1.12      0.55 / 1.15   0.97 / 0.82
    float32  restated = dca_numpy, driver 1 worker   1.63      0.89      2.18
             NumpyBackend driver, 4 workers          1.63      1.29      2.34
             HIP driver, 1 / 4 workers               1.63      1.29      2.73 / 1.24
(alpha is the same pass everywhere -- the kernel gives the stated order's bytes; the runs differ in the order in which
the expression for w adds the rows.)  The largest is 2.73 of the 8 allowed.  Training accuracy on the golden input after
3 iterations: 0.946 (140 of 148), the yardstick's w and every run of ours alike.

NaN.  "Byte for byte" holds for every value that is not a NaN.  The sign and payload of a NaN that an operation makes
or passes on differ between processors (0 * inf is 0xfff8... on x86 and 0x7ff8... on the GPU), so `same` compares NaN
by position and everything else by its bytes.
"""
import os

import numpy as np

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'disdca_svm_w4.npz')

# the golden recipe
N, D, WORKERS, ITERS, LA = 148, 7, 4, 3, 0.1
FACTOR = 8.0
F32_OVER_F64 = 2.0 ** 29

# the device shapes: m on both sides of the ring's batches and of 64; d on both sides of every bucket of
# ceil(d / 64) = 1, 2, 4, 8, 16 (registers) and 32, 64 (LDS)
MS = (0, 1, 2, 63, 64, 65, 200)
DS = (1, 3, 63, 64, 65, 130, 1000)
BIG_D = (5, 4096)             # (m, d)


def same(got, want):
  """Equal byte for byte, a NaN standing for any NaN."""
  got, want = np.asarray(got), np.asarray(want)
  if got.shape != want.shape or got.dtype != want.dtype:
    return False
  gn, wn = np.isnan(got), np.isnan(want)
  return bool((gn == wn).all()) and np.where(gn, 0, got).tobytes() == np.where(wn, 0, want).tobytes()


def golden_input():
  """(X [148, 7] float64, y [148, 1] int64 of +1 / -1): the recipe of the golden."""
  rng = np.random.RandomState(5)
  x = rng.randn(N, D)
  y = np.where(x[:, 0] > x[:, 1] + 0.3 * rng.randn(N), 1, -1).reshape(N, 1).astype(np.int64)
  return x, y


def case(m, d, dtype, seed=0):
  """(x [m, d], y [m] of +1 / -1, alpha [m] inside [0, 1] y, w0 [d] not zero, scaled_lambda) in `dtype`; the rows have
  norms near 1 so that every branch of the clamp is taken."""
  dt = np.dtype(dtype)
  rng = np.random.RandomState(1000 * seed + 7 * m + d)
  x = (rng.randn(m, d) / np.sqrt(d)).astype(dt)
  truth = rng.randn(d)
  y = np.where(x.astype(np.float64).dot(truth) + 0.2 * rng.randn(m) >= 0, 1, -1).astype(dt)
  alpha = (rng.rand(m) * (rng.rand(m) < 0.7)).astype(dt) * y
  w0 = (0.3 * rng.randn(d)).astype(dt)
  return x, y, alpha, w0, 0.75


SPECIAL_SCALE, SPECIAL_LAMBDA_N = 2, 0.1 * 12      # the reference's `scale` and `lambda_n` for the special rows
SPECIAL_ROWS = {'zero row': 1, 'y = 0': 3, 'zero row with y = 0': 5, 'alpha above y': 6, 'alpha of the other sign': 7,
                'norm 1e-200': 8, 'NaN in x': 10}


def special_case(dtype=np.float64):
  """(x [12, 7], y [12], alpha [12], w0 [7], scaled_lambda) with the rows of SPECIAL_ROWS; the row after the NaN shows
  that later rows keep running.  (In float32 the row of norm 1e-200 is a row of zeros.)"""
  rng = np.random.RandomState(11)
  x = rng.randn(12, 7) / np.sqrt(7)
  y = np.where(rng.rand(12) < 0.5, 1.0, -1.0)
  alpha = rng.rand(12) * y * 0.5
  w0 = 0.3 * rng.randn(7)
  x[1] = 0
  y[3] = 0
  x[5], y[5] = 0, 0
  alpha[6] = 3.5 * y[6]
  alpha[7] = -2.0 * y[7]
  x[8] = 1e-200 * rng.randn(7)
  x[10, 3], x[10, 5] = np.nan, 0.0
  dt = np.dtype(dtype)
  return x.astype(dt), y.astype(dt), alpha.astype(dt), w0.astype(dt), SPECIAL_SCALE * 1.0 / SPECIAL_LAMBDA_N


def chain_rows(m, chains):
  return [(c * m // chains, (c + 1) * m // chains) for c in range(chains)]


def stated_dot(p, r):
  """dot(p, r) in the header's order, scalar by scalar in the vectors' dtype."""
  zero = p.dtype.type(0)
  sums = []
  for lane in range(64):
    acc = zero
    for a, b in zip(p[lane::64], r[lane::64]):
      acc = acc + a * b
    sums.append(acc)
  for s in (32, 16, 8, 4, 2, 1):
    sums = [sums[i] + sums[i + s] for i in range(s)]
  return sums[0]


def restated(x, y, alpha, w0, scaled_lambda, chains=1):
  """(alpha' [m], w [chains, d]) of one pass in the stated order, every operation in x's dtype."""
  dt = x.dtype
  m, d = x.shape
  s, one, zero = dt.type(scaled_lambda), dt.type(1), dt.type(0)
  out, w_out = np.array(alpha.reshape(m)), np.empty((chains, d), dt)
  y, alpha = y.reshape(m), alpha.reshape(m)
  with np.errstate(all='ignore'):
    for c, (lo, hi) in enumerate(chain_rows(m, chains)):
      w = np.array(w0.reshape(d))
      for i in range(lo, hi):
        big_a = s * stated_dot(x[i], x[i])
        t = y[i] - stated_dot(x[i], w)
        g = t / big_a
        v = y[i] * (g + alpha[i])
        c1 = v if v < one else one
        c2 = c1 if c1 > zero else zero
        dl = y[i] * c2 - alpha[i]
        for j in range(d):
          w[j] = w[j] + (x[i, j] * s) * dl
        out[i] = alpha[i] + dl
      w_out[c] = w
  assert out.dtype == dt and w_out.dtype == dt
  return out, w_out


def yardstick(x, y, alpha, w0, scaled_lambda, chains=1):
  """The same recurrence in longdouble with plain sums: (alpha' [m], w [chains, d]) as longdouble arrays."""
  m, d = x.shape
  # (scaled_lambda is rounded to the arrays' dtype first: that rounding is part of the contract, not of the error)
  s = LD(x.dtype.type(scaled_lambda))
  x, y, alpha, w0 = (np.asarray(a, LD) for a in (x, y.reshape(m), alpha.reshape(m), w0.reshape(d)))
  out, w_out = np.array(alpha), np.empty((chains, d), LD)
  with np.errstate(all='ignore'):
    for c, (lo, hi) in enumerate(chain_rows(m, chains)):
      w = np.array(w0)
      for i in range(lo, hi):
        g = (y[i] - np.dot(x[i], w)) / (s * np.dot(x[i], x[i]))
        v = y[i] * (g + alpha[i])
        c1 = v if v < 1 else LD(1)
        c2 = c1 if c1 > 0 else LD(0)
        dl = y[i] * c2 - alpha[i]
        w = w + (x[i] * s) * dl
        out[i] = alpha[i] + dl
      w_out[c] = w
  return out, w_out


def run(body, x, y, iters=ITERS, la=LA, bands=WORKERS, chains=1, dtype=np.float64):
  """A whole fit with `body` as the pass: ([alpha after every iteration], w after the last), alpha [n], w [d]; in
  `dtype`, or in longdouble on the `dtype`-rounded inputs where body is `yardstick`."""
  dt = np.dtype(dtype)
  n, d = x.shape
  x, y = np.asarray(x, dt), np.asarray(y, dt).reshape(n)
  band = max(-(-n // bands), 1)
  cuts = [(lo, min(lo + band, n)) for lo in range(0, n, band)]
  scaled_lambda = len(cuts) * chains * 1.0 / (la * n)
  wide = body is yardstick
  work = LD if wide else dt.type
  w, alpha, alphas = np.zeros(d, x.dtype), np.zeros(n, x.dtype), []
  if wide:
    w, alpha = w.astype(LD), alpha.astype(LD)
  for _ in range(iters):
    new = np.empty_like(alpha)
    for lo, hi in cuts:
      if wide:
        new[lo:hi] = _yardstick_wide(x[lo:hi], y[lo:hi], alpha[lo:hi], w, scaled_lambda, chains)
      else:
        new[lo:hi] = np.asarray(body(x[lo:hi], y[lo:hi], alpha[lo:hi], w, scaled_lambda, chains)[0]).reshape(hi - lo)
    alpha = new
    xa = np.asarray(x, LD) if wide else x
    w = (xa * alpha[:, None] * work(1.0) / work(dt.type(la)) / work(dt.type(n))).sum(axis=0)
    alphas.append(alpha)
  assert wide or (w.dtype == dt and alpha.dtype == dt)
  return alphas, w


def _yardstick_wide(x, y, alpha, w0, scaled_lambda, chains):
  """yardstick on a band whose alpha and w0 are longdouble already (they are not rounded between iterations)."""
  m, d = x.shape
  s = LD(x.dtype.type(scaled_lambda))
  xl, yl = np.asarray(x, LD), np.asarray(y, LD)
  out = np.array(alpha)
  for lo, hi in chain_rows(m, chains):
    w = np.array(w0)
    for i in range(lo, hi):
      g = (yl[i] - np.dot(xl[i], w)) / (s * np.dot(xl[i], xl[i]))
      v = yl[i] * (g + alpha[i])
      c1 = v if v < 1 else LD(1)
      c2 = c1 if c1 > 0 else LD(0)
      dl = yl[i] * c2 - alpha[i]
      w = w + (xl[i] * s) * dl
      out[i] = alpha[i] + dl
  return out


_cache = {}


def golden():
  if 'golden' not in _cache:
    _cache['golden'] = dict(np.load(GOLDEN))
  return _cache['golden']


def golden_yardstick(dtype=np.float64):
  """{'alpha_1', 'alpha_3', 'w_3'} of the yardstick on the golden input (rounded to `dtype`), computed once."""
  key = ('yardstick', np.dtype(dtype).name)
  if key not in _cache:
    x, y = golden_input()
    alphas, w = run(yardstick, x, y, dtype=dtype)
    _cache[key] = {'alpha_1': alphas[0], 'alpha_3': alphas[-1], 'w_3': w}
  return _cache[key]


def e_ref():
  """{'alpha_1', 'alpha_3', 'w_3'}: the largest absolute distance of the golden's recorded array to the yardstick."""
  g, want = golden(), golden_yardstick()
  return {k: float(np.abs(np.asarray(g[k], LD).reshape(-1) - want[k]).max()) for k in want}


def check_accuracy(got, dtype, label):
  """`got` = {'alpha_1', 'alpha_3', 'w_3'} of a run of ours in `dtype` on the golden input: prints every ratio to e_ref
  (over 2^29 in float32), then asserts the rule.  Returns the ratios."""
  dt = np.dtype(dtype)
  want, ref = golden_yardstick(dt), e_ref()
  scale = F32_OVER_F64 if dt == np.float32 else 1.0
  ratios = {}
  for k in ('alpha_1', 'alpha_3', 'w_3'):
    assert ref[k] > 0, (k, ref)
    err = float(np.abs(np.asarray(got[k], LD).reshape(-1) - want[k]).max())
    ratios[k] = err / (ref[k] * scale)
    print('%s %s %s: max abs distance to the yardstick %.3g, e_ref %.3g, ratio %.3g (limit %g)'
          % (label, dt.name, k, err, ref[k], ratios[k], FACTOR))
  assert all(r <= FACTOR for r in ratios.values()), (label, ratios)
  return ratios
