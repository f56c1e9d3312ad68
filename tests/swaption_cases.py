"""Cases, oracle and error bound of the swaption tests (sp_lmm_swaption, examples/_swaption.py, examples/swaption.py).  No
test functions.

Oracle.  `oracle` is a literal NumPy transcription of the reference's array program (spartan/examples/swaption.py:
47-97) for one product, written in S = ts / delta steps and K = te / delta maturities: the draws concatenated with their
negatives, the [maturities, 2 paths] plane that loses its first row every step, `mu` as the cumsum over axis 0, the
`zcb` and `b_ts` loops, the final halves added.  Its scalars are converted to the draws' dtype T first, so that it runs
in T; the reference itself is float64.

Bound.  `bound(eps, K, lamb, ...)` is derived, not measured: per pair, an absolute bound on the difference between two
implementations of the recurrence of include/spartan_hip_lmm.h in T whose every operation but exp is IEEE and whose exp
is within 2 ulp of the exact exp of its (computed) argument -- the figure tests/fuzzy_cases.py takes for pow; HIP's
documentation of its device math functions gives 1 ulp for expf and exp.  It is twice `forward_bound`, the distance of
one such implementation from the exact value of the recurrence on the same T inputs: |a - b| <= |a - x| + |b - x|.
With u the unit roundoff of T (2^-24, 2^-53), factors composed and never added, for every sign:
  c0, sq, cth   three, one and one rounding: (1 + u)^3, (1 + u), (1 + u).
  f[k]          carries a relative bound r_k (0 at the start: F is a value of T).  Within step t:
                  df = D f[k]            1 + r_df = (1 + r_k)(1 + u)
                  1 + df                 the 1 is exact and df > 0: 1 + r_g = (1 + r_df df / (1 + df))(1 + u)
                  term = (lam df) / (1 + df)     1 + r_term = (1 + r_df)(1 + u)(1 + u) / (1 - r_g)
                  mu_k                   a sum of k - t + 1 positive terms, k - t roundings:
                                         1 + r_mu = (1 + max_j r_term_j)(1 + u)^(k - t)
                  a = ((lam mu) D - c0) + z      an ABSOLUTE bound: A1 = |lam mu D| ((1 + r_mu)(1 + u)^2 - 1),
                                         Ac = |c0| ((1 + u)^3 - 1), the difference rounds: A2 = A1 + Ac + u (|a1 - c0| + A1 +
                                         Ac); Az = |z| ((1 + u)^3 - 1) (two products and sq); the sum rounds:
                                         A = A2 + Az + u (|a| + A2 + Az)
                  exp                    1 + r_e = e^A (1 + 4 u)
                  f[k] <- f[k] exp(a)    1 + r_k' = (1 + r_k)(1 + r_e)(1 + u)
  b             1 + r_b' = (1 + r_b)(1 + r_g of f[t-1])(1 + u) per step
  zc            relative through the chain, 1 + r_z' = (1 + r_z)(1 + u) / (1 - r_g of f[k]); then absolute, Z = r_z zc
  acc           absolute: C' = C + Z + u (acc + C + Z) per addition (the first adds to an exact 0)
  x             1 - zc: X1 = Z + u (|1 - zc| + Z);  cth acc: X2 = cth acc ((1 + u)^2 (1 + C / acc) - 1);
                the subtraction: X = X1 + X2 + u (|x| + X1 + X2).  max(., 0) is 1-Lipschitz: X passes through it.
  v = m / b     V = (m + X)(1 + u) / (b (1 - r_b)) - m / b = (m / b)((1 + u) / (1 - r_b) - 1) + X (1 + u) / (b (1 - r_b))
  out           (v+ + v-) / 2: (V+ + V- + u (v+ + v- + V+ + V-)) / 2; the halving is exact.
The magnitudes (df, mu, a, zc, acc, x, m, b) are those of a float64 run of the recurrence, each enlarged by 1e-6 where
it multiplies a bound: the float64 run's own error is orders below that.  The derivation needs lam >= 0, D > 0 and
F > 0 (positive rates, positive terms) and finite draws; `forward_bound` asserts them.
Two conditions keep the bound from hiding a failure, and tests/test_swaption_cases_cpu.py checks both for every case
used: it stays below 1 % (float32) and 1e-9 (float64) of the case's mean payoff, and the float32 NumPy body against the
float64 oracle -- an implementation whose exp is NumPy's -- lies inside it."""
import os

import numpy as np

from spartan_amd import _hip

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'swaption_w4.npz')

DELTA, F_0, THETA = 0.5, 0.06, 0.06         # the reference's parameter values
MAX_K = _hip.SP_LMM_MAX_K
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
CAP = {np.dtype(np.float32): 1e-2, np.dtype(np.float64): 1e-9}     # of the case's mean payoff

# the reference's benchmark (tests/benchmark_swaption.py), in simulate's iteration order
TS_ALL = [[1, 2, 3], [2, 3, 4], [5, 6, 7, 8, 9], [10, 12, 14, 16, 18]]
TE_ALL = [4, 5, 10, 20]
LAMB_ALL = [0.2, 0.2, 0.15, 0.1]
NUM_PATHS = 10
WORKERS = 4


def products():
  """[(ts, te, lamb)] of the benchmark, in the order simulate walks them."""
  return [(ts, te, lamb) for ts_a, te, lamb in zip(TS_ALL, TE_ALL, LAMB_ALL) for ts in ts_a]


def steps_of(ts, te, delta=DELTA):
  """(S, K) of a product."""
  return int(round(ts / delta)), int(round(te / delta))


# the sizes of the GPU tests: n around the 64 lanes of a workgroup, more than one workgroup, a partly filled last one
NS = (1, 2, 63, 64, 65, 257, 600)
N_SHAPE = (2, 8, 0.2)
# (S, K, lamb) at n = 65: the smallest, the last step before the last maturity, the reference's widest plane at its two
# ends and its middle, the widest the kernel takes at its two ends.  lamb is 0.2 except for the 127 steps of 128
# maturities: there the drift lam mu D of 127 maturities feeds on the rates it raises, at 0.2 the rates of half the
# pairs overflow float64 in the oracle itself and no bound exists; 0.05 continues the reference's own products (0.2 at 4
# and 5 years, 0.15 at 10, 0.1 at 20) to 64 years and keeps every rate below 1.
SHAPES = ((1, 2, 0.2), (7, 8, 0.2), (1, 40, 0.2), (36, 40, 0.2), (20, 40, 0.2), (1, MAX_K, 0.2), (MAX_K - 1, MAX_K, 0.05))


def draws(s, n, dtype, seed=0):
  """[s, n] standard normal draws in `dtype`, a function of (s, n, seed) alone."""
  rng = np.random.RandomState(20151107 + 1000 * seed + 7 * s + n)
  return np.ascontiguousarray(rng.randn(s, n).astype(dtype))


def oracle(eps_tmp, maturities, lamb, delta=DELTA, f0=F_0, theta=THETA):
  """The reference's array program for one product on the draws eps_tmp [S, num_paths], in their dtype: [num_paths]
  values, (swaption[0:num_paths] + swaption[num_paths:]) / 2 of swaption.py:96.  The comments name its lines."""
  dt = eps_tmp.dtype
  n_steps, num_paths = eps_tmp.shape
  k_n = int(maturities)
  lamb, DELTA_, F_0_, THETA_ = (dt.type(v) for v in (lamb, delta, f0, theta))
  one, half, zero = dt.type(1), dt.type(0.5), dt.type(0)
  with np.errstate(all='ignore'):
    eps = np.concatenate([eps_tmp, -eps_tmp], 1)                      # eps = concatenate(eps_tmp, -eps_tmp, 1)
    f_kk = np.zeros((n_steps + 1, 2 * num_paths), dt)                 # f_kk = zeros((time_structure.shape[0], 2 N))
    f_kk[0, :] = F_0_                                                 # f_kk = assign(f_kk, np.s_[0, :], F_0)
    f_kn = np.ones((k_n, 2 * num_paths), dt) * F_0_                   # f_kn = ones((maturities, 2 N)) * F_0
    for t in range(1, n_steps + 1):
      tmp = lamb * (DELTA_ * f_kn[1:, :]) / (one + DELTA_ * f_kn[1:, :])          # mu(f, lamb)
      mu = np.cumsum(tmp, axis=0)                                     # spartan.scan(tmp, np.sum, np.cumsum, axis=0)
      f_kn_new = f_kn[1:, :] * np.exp(lamb * mu * DELTA_ - half * lamb * lamb * DELTA_
                                      + lamb * eps[t - 1, :] * np.sqrt(DELTA_))
      f_kk[t, :] = f_kn_new[0]                                        # f_kk = assign(f_kk, np.s_[t, :], f_kn_new[0])
      f_kn = f_kn_new
    zcb = np.ones((k_n - n_steps + 1, 2 * num_paths), dt)             # zcb = ones((int((te - ts) / DELTA) + 1, 2 N))
    f_kn_modified = one + DELTA_ * f_kn
    for j in range(zcb.shape[0] - 1):
      zcb[j + 1] = zcb[j] / f_kn_modified[j]
    last_row = zcb[zcb.shape[0] - 1, :].reshape((2 * num_paths,))
    swap_ts = np.maximum(one - last_row - THETA_ * DELTA_ * np.sum(zcb[1:], 0), zero)
    b_ts = np.ones((2 * num_paths,), dt)
    tmp = one + DELTA_ * f_kk
    for j in range(n_steps):                                          # for j in xrange(int(ts / DELTA))
      b_ts *= tmp[j].reshape((2 * num_paths,))
    swaption = swap_ts / b_ts
    out = (swaption[0:num_paths] + swaption[num_paths:]) / dt.type(2)
  assert out.dtype == dt and f_kn.dtype == dt and zcb.dtype == dt and b_ts.dtype == dt
  return out


def forward_bound(eps, maturities, lamb, delta=DELTA, f0=F_0, theta=THETA, exp_ulps=2.0):
  """[n] absolute bounds on |out^ - out| for an implementation of the recurrence in the dtype of `eps` (the module
  docstring's derivation, line for line), float64."""
  dt = np.dtype(eps.dtype)
  u = U[dt]
  s_n, n = eps.shape
  k_n = int(maturities)
  lam, d, f_0, th = (float(dt.type(v)) for v in (lamb, delta, f0, theta))
  assert lam >= 0 and d > 0 and f_0 > 0 and np.isfinite(eps).all()
  up = 1 + 1e-6                    # what a float64 magnitude is enlarged by where it multiplies a bound
  e64 = np.asarray(eps, np.float64)
  c0, sq, cth = 0.5 * lam * lam * d, np.sqrt(d), th * d
  r3 = (1 + u) ** 3 - 1
  v, big_v = [], []
  for sign in (1.0, -1.0):
    f = np.full((k_n, n), f_0)
    r = np.zeros((k_n, n))

    def r_g(k):                    # of 1 + D f[k]
      df = d * f[k] * up
      return (1 + ((1 + r[k]) * (1 + u) - 1) * df / (1 + df)) * (1 + u) - 1

    b, r_b = np.ones(n), np.zeros(n)
    for t in range(1, s_n + 1):
      r_b = (1 + r_b) * (1 + r_g(t - 1)) * (1 + u) - 1
      b = b * (1 + d * f[t - 1])
      z = lam * (sign * e64[t - 1]) * sq
      mu, r_term_max = np.zeros(n), np.zeros(n)
      for k in range(t, k_n):
        r_df = (1 + r[k]) * (1 + u) - 1
        r_term = (1 + r_df) * (1 + u) * (1 + u) / (1 - r_g(k)) - 1
        r_term_max = np.maximum(r_term_max, r_term)
        df = d * f[k]
        mu = mu + lam * df / (1 + df)
        r_mu = (1 + r_term_max) * (1 + u) ** (k - t) - 1
        a1 = lam * mu * d
        big_a1 = np.abs(a1) * up * ((1 + r_mu) * (1 + u) ** 2 - 1)
        big_c = abs(c0) * up * r3
        big_a2 = big_a1 + big_c + u * (np.abs(a1 - c0) * up + big_a1 + big_c)
        big_z = np.abs(z) * up * r3
        a = (a1 - c0) + z
        big_a = big_a2 + big_z + u * (np.abs(a) * up + big_a2 + big_z)
        r_e = np.exp(big_a) * (1 + 2 * exp_ulps * u) - 1
        r[k] = (1 + r[k]) * (1 + r_e) * (1 + u) - 1
        f[k] = f[k] * np.exp(a)
    zc, r_z, acc, big_c = np.ones(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for k in range(s_n, k_n):
      r_z = (1 + r_z) * (1 + u) / (1 - r_g(k)) - 1
      zc = zc / (1 + d * f[k])
      big_z = r_z * zc * up
      big_c = big_c + big_z + (u * (acc + zc + big_c + big_z) * up if k > s_n else 0.0)
      acc = acc + zc
    x = (1 - zc) - cth * acc
    x1 = big_z + u * (np.abs(1 - zc) * up + big_z)
    x2 = cth * acc * up * ((1 + u) ** 2 * (1 + big_c / acc) - 1)
    big_x = x1 + x2 + u * (np.abs(x) * up + x1 + x2)
    m = np.maximum(x, 0.0)
    v.append(m / b)
    big_v.append((m / b) * up * ((1 + u) / (1 - r_b) - 1) + big_x * (1 + u) * up / (b * (1 - r_b)))
  return (big_v[0] + big_v[1] + u * ((v[0] + v[1]) * up + big_v[0] + big_v[1])) / 2


def bound(eps, maturities, lamb, delta=DELTA, f0=F_0, theta=THETA):
  """[n] absolute bounds on the difference of two implementations of the recurrence in the dtype of `eps` -- the kernel
  and the oracle, or the NumPy body and the oracle: twice forward_bound."""
  return 2 * forward_bound(eps, maturities, lamb, delta, f0, theta)


def share(got, want, limit):
  """The largest |got - want| / limit over the pairs: what the tests print before they assert it is at most 1."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape == limit.shape and np.isfinite(got).all() and (limit > 0).all()
  return float((np.abs(got - want) / limit).max())


def golden():
  """The recorded run of the reference at 4 workers (tests/golden/make_golden_swaption.py): a dict with `products`
  [16, 3] (ts, te, lamb), `results` [16, 2] (mean, std in basis points), `whole_run` and `eps_all`, the list of the 16
  draw arrays [S, 10]."""
  z = np.load(GOLDEN)
  prods = z['products']
  return {'products': prods, 'results': z['results'], 'whole_run': int(z['whole_run']),
          'eps_all': [np.array(z['eps_%02d' % i]) for i in range(len(prods))]}
