"""The tile body of the swaption driver: backend.lmm_swaption where the backend has it (HipBackend: sp_lmm_swaption),
NumPy on host arrays otherwise -- the same recurrence, operation for operation in the draws' dtype
(include/spartan_hip_lmm.h), which keeps the driver runnable on a backend of plain NumPy tiles.  Everything but `exp`
is an IEEE operation on both sides, so NumPy's exp against the device library's is all that separates the two.  Both
paths refuse through one function, tile_checks.check_lmm_swaption (the launcher and HipBackend.lmm_swaption call it
too)."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray

check_operands = tile_checks.check_lmm_swaption


def payoffs_numpy(eps, maturities, lamb, delta, f0, theta):
  """out [n] in the dtype T of the draws eps [S, n]: per antithetic pair p, for the sign s = +1 and then s = -1, with
  lam, D, F, TH the four scalars in T, c0 = ((T(0.5) lam) lam) D, sq = sqrt(D), cth = TH D, every operation rounded once
  in T,
      f[0 .. K-1] = F;  b = 1
      for t = 1 .. S:   b = b (1 + D f[t-1]);   z = (lam (s eps[t-1, p])) sq
                        for k = t .. K-1:  mu_k = mu_{k-1} + (lam (D f[k])) / (1 + D f[k])   (a running sum from mu_t = its
                                           f[k] = f[k] exp(((lam mu_k) D - c0) + z)            own term: numpy.cumsum)
      zc = 1; acc = 0;  for k = S .. K-1:  zc = zc / (1 + D f[k]);  acc = acc + zc
      v_s = maximum((1 - zc) - cth acc, 0) / b
  and out[p] = (v_+ + v_-) / 2.  Vectorised over the pairs with element-wise operations and a cumsum down the
  maturities only, on arrays that are contiguous where exp meets them: a pair's bits do not depend on its neighbours.
  `eps` is not written."""
  dt = eps.dtype
  s_n, n = eps.shape
  k_n = int(maturities)
  lam, d, f_0, th = (dt.type(v) for v in (lamb, delta, f0, theta))
  one, zero = dt.type(1), dt.type(0)
  v = []
  with np.errstate(all='ignore'):
    c0 = ((dt.type(0.5) * lam) * lam) * d
    sq = np.sqrt(d)
    cth = th * d
    for sign in (1, -1):
      f = np.full((k_n, n), f_0, dt)
      b = np.full((n,), one, dt)
      for t in range(1, s_n + 1):
        b = b * (one + d * f[t - 1])
        draw = eps[t - 1] if sign > 0 else -eps[t - 1]
        z = (lam * draw) * sq
        df = d * f[t:]
        mu = np.cumsum((lam * df) / (one + df), axis=0)
        f[t:] = f[t:] * np.exp(np.ascontiguousarray(((lam * mu) * d - c0) + z[None, :]))
      zc, acc = np.full((n,), one, dt), np.zeros((n,), dt)
      for k in range(s_n, k_n):
        zc = zc / (one + d * f[k])
        acc = acc + zc
      v.append(np.maximum((one - zc) - cth * acc, zero) / b)
    out = (v[0] + v[1]) / dt.type(2)
  assert out.dtype == dt and f.dtype == dt and b.dtype == dt and mu.dtype == dt
  return out


def lmm_swaption(eps, maturities, lamb, delta=0.5, f0=0.06, theta=0.06):
  """The discounted payoffs [n] of one swaption as a new tile, from the draws `eps` [S, n], float32 or float64.
  TypeError ("astype first") for other dtypes, ValueError for draws that are not 2-D, S and K = `maturities` that do not
  satisfy 1 <= S < K <= SP_LMM_MAX_K, scalars that are not finite and delta <= 0."""
  if isinstance(eps, distarray.Absent):
    dt, n = check_operands(eps.dtype, eps.shape, maturities, lamb, delta, f0, theta)[:2]
    return distarray.Absent((n,), dt)
  be = context.get().backend
  fn = getattr(be, 'lmm_swaption', None)
  if fn is not None:
    return fn(eps, maturities, lamb, delta=delta, f0=f0, theta=theta)
  host = np.asarray(be.to_numpy(eps))
  _, _, _, k, lamb, delta, f0, theta = check_operands(host.dtype, host.shape, maturities, lamb, delta, f0, theta)
  return payoffs_numpy(host, k, lamb, delta, f0, theta)
