"""European payer swaptions under Andersen's LIBOR market model by Monte Carlo with antithetic paths (interface of the
reference's spartan/examples/swaption.py: `simulate(ts_all, te_all, lamb_all, num_paths)` -> a list of [mean, std] in
basis points, one per product, and the constants DELTA, F_0, THETA; its tests/benchmark_swaption.py prices 16 products
with 10 paths).

A product (ts, te, lamb) has S = ts / DELTA time steps and K = te / DELTA forward rates, all F_0 at the start.  Per path,
with standard normal draws eps[t] (swaption.py:56-97):

    step t = 1 .. S:   mu_k = sum over j = t .. k of lamb DELTA f_j / (1 + DELTA f_j)
                       f_k  = f_k exp(lamb mu_k DELTA - lamb^2 DELTA / 2 + lamb eps[t-1] sqrt(DELTA))     for k = t .. K-1
    zcb_k = product over j = S .. k of 1 / (1 + DELTA f_j);   swap = max(1 - zcb_{K-1} - THETA DELTA sum_k zcb_k, 0)
    payoff = swap / product over t = 0 .. S-1 of (1 + DELTA f_t as it stood after step t)

and every path runs a second time with the negated draws; v = the mean of the two.  The product's result is
[mean(v) 10000, std(v) / sqrt(num_paths) 10000].

The reference walks a [maturities, 2 paths] plane through the steps -- a scan, an exp map, a slice and an assign per
step, two loops of assign / *= per product.  method='fused' (the default) draws randn(S, num_paths) tiled into column
bands of divup(num_paths, workers) and runs ONE shuffle over the bands whose tile body is one _swaption.lmm_swaption
per band (HipBackend: sp_lmm_swaption -- all steps of a pair of paths in one kernel, the rates on chip, nothing of size
maturities x paths allocated) into a (num_paths,) target; mean and std are the reference's own expressions on the map
and reduce kernels.  include/spartan_hip_lmm.h states the recurrence operation for operation; in NumPy float64 it gives
the reference's array program's bytes per pair.  method='expr' is the reference's program, line for line, on the
expression builders (its two reshape((20, )), which hard-code 10 paths, written as reshape((2 * num_paths, ))); it is
kept for comparison and for the benchmark.

Additions: `method`; `dtype` (float64 as the reference, or float32: the draws are converted with astype and the paths
run in float32; std casts to float64 as the library's std does); `eps_all`, one [S, num_paths] array per product in
simulate's iteration order (NumPy arrays or distributed arrays) in place of the draws -- the reference draws from
NumPy's generator and this library from its own, so a recorded run can only be repeated on its own draws; `delta`,
`f0`, `theta` (the reference's module constants).  Deviations: dates that are not whole multiples of `delta` or that do
not satisfy 0 < ts < te raise ValueError (the reference's three length formulas -- arange(0, ts + DELTA, DELTA),
int((te - ts) / DELTA) + 1 and int(ts / DELTA) -- disagree for such dates), as do more than SP_LMM_MAX_K maturities,
num_paths < 1, a bad method, an eps_all of another length or shape and scalars that are not finite; a dtype other than
the two raises TypeError.  The reference's `print i` is dropped."""
import numpy as np

from .. import context, expr, tile_checks, util
from ..array import extent
from . import _swaption

# Parameter Values.
DELTA = 0.5
F_0 = 0.06
THETA = 0.06

METHODS = ('fused', 'expr')


def _payoff_mapper(array, ex, maturities=None, lamb=None, delta=None, f0=None, theta=None):
  """Tile body of a product: the payoffs of this band of pairs, as the band's elements of the (num_paths,) target."""
  if ex.ul[0] != 0:                     # (a band cut by rows as well: its first tile speaks for all of them)
    return []
  lo, hi = ex.ul[1], ex.lr[1]
  steps, n = array.shape
  eps = array.fetch(extent.create((0, lo), (steps, hi), array.shape))
  return [(extent.create((lo,), (hi,), (n,)),
           _swaption.lmm_swaption(eps, maturities, lamb, delta=delta, f0=f0, theta=theta))]


_payoff_mapper.yields_fresh_tensors = True      # the kernel's output (or NumPy's), never a fetched tile


def _grid(ts, te, delta):
  """(S, K) of a product, or ValueError for dates off the grid of `delta` or not satisfying 0 < ts < te."""
  ts, te = float(ts), float(te)
  if not 0 < ts < te or te == float('inf'):
    raise ValueError('simulate: dates ts = %r, te = %r must satisfy 0 < ts < te' % (ts, te))
  s, k = int(round(ts / delta)), int(round(te / delta))
  for name, date, steps in (('ts', ts, s), ('te', te, k)):
    if abs(steps * delta - date) > 1e-9 * date:
      raise ValueError('simulate: %s = %r is not a whole multiple of delta = %r' % (name, date, delta))
  return s, k


def _draws(eps, steps, num_paths, band, dtype):
  """The draws of a product as an evaluated distributed array [steps, num_paths] of `dtype` in column bands."""
  if eps is None:
    eps = expr.randn(steps, num_paths, tile_hint=(steps, band))
  elif isinstance(eps, np.ndarray):
    if eps.shape != (steps, num_paths):
      raise ValueError('simulate: eps_all holds draws of shape %s for a product of %d steps and %d paths'
                       % (eps.shape, steps, num_paths))
    if eps.dtype.kind not in 'fiub':
      raise TypeError('simulate: draws of dtype %s; the draws are real numbers' % eps.dtype)
    eps = expr.from_numpy(eps, tile_hint=(steps, band))
  else:
    if tuple(eps.shape) != (steps, num_paths):
      raise ValueError('simulate: eps_all holds draws of shape %s for a product of %d steps and %d paths'
                       % (tuple(eps.shape), steps, num_paths))
    eps = expr.retile(eps, tile_hint=(steps, band))
  eps = expr.evaluate(eps)
  if np.dtype(eps.dtype) != dtype:
    eps = expr.evaluate(expr.astype(eps, dtype))
  return eps


def _fused(eps, steps, maturities, num_paths, band, lamb, dtype, delta, f0, theta):
  """(swaption[0:num_paths] + swaption[num_paths:]) / 2 of swaption.py:96 as an evaluated (num_paths,) array."""
  target = expr.ndarray((num_paths,), dtype=dtype, tile_hint=(band,))
  return expr.shuffle(eps, _payoff_mapper, target=target,
                      kw={'maturities': maturities, 'lamb': lamb, 'delta': delta, 'f0': f0, 'theta': theta}).evaluate()


def _expr(eps_tmp, steps, maturities, num_paths, lamb, dtype, delta, f0, theta):
  """The reference's program (swaption.py:56-96) on the expression builders; the comments name its lines.  Scalars are
  values of `dtype` (Python scalars would promote float32)."""
  lamb, delta, f0, theta = (dtype.type(v) for v in (lamb, delta, f0, theta))
  one, half = dtype.type(1), dtype.type(0.5)
  eps_tmp = expr.lazify(eps_tmp)
  eps = expr.concatenate(eps_tmp, -eps_tmp, 1)                       # eps = concatenate(eps_tmp, -eps_tmp, 1)
  f_kk = expr.zeros((steps + 1, 2 * num_paths), dtype=dtype)          # f_kk = zeros((time_structure.shape[0], 2 N))
  f_kk = expr.assign(f_kk, np.s_[0, :], float(f0))                    # f_kk = assign(f_kk, np.s_[0, :], F_0)
  f_kn = expr.ones((maturities, 2 * num_paths), dtype=dtype) * f0     # f_kn = ones((maturities, 2 N)) * F_0
  for t in range(1, steps + 1):
    tmp = lamb * (delta * f_kn[1:, :]) / (one + delta * f_kn[1:, :])  # mu(f, lamb)
    mu = expr.scan(tmp, np.sum, np.cumsum, axis=0)
    f_kn_new = f_kn[1:, :] * expr.exp(lamb * mu * delta - half * lamb * lamb * delta
                                      + lamb * eps[t - 1, :] * np.sqrt(delta))
    f_kk = expr.assign(f_kk, np.s_[t, :], f_kn_new[0])
    f_kn = f_kn_new
  zcb = expr.ones((maturities - steps + 1, 2 * num_paths), dtype=dtype)
  f_kn_modified = one + delta * f_kn
  for j in range(zcb.shape[0] - 1):
    zcb = expr.assign(zcb, np.s_[j + 1], zcb[j] / f_kn_modified[j])
  last_row = zcb[zcb.shape[0] - 1, :].reshape((2 * num_paths,))
  swap_ts = expr.maximum(one - last_row - theta * delta * expr.sum(zcb[1:], 0), dtype.type(0))
  b_ts = expr.ones((2 * num_paths,), dtype=dtype)
  tmp = one + delta * f_kk
  for j in range(steps):
    b_ts *= tmp[j].reshape((2 * num_paths,))
  swaption = swap_ts / b_ts
  return (swaption[0:num_paths] + swaption[num_paths:]) / dtype.type(2)


def simulate(ts_all, te_all, lamb_all, num_paths, method='fused', dtype=np.float64, eps_all=None, delta=DELTA, f0=F_0,
             theta=THETA):
  """Range over a number of independent products: for every end date te of `te_all`, with its volatility from
  `lamb_all`, one swaption per start date of its entry of `ts_all` (a list of lists), each priced with `num_paths`
  antithetic pairs of paths.  Returns the reference's list of [mean, std], both evaluated distributed scalars in basis
  points (`.glom()` gives the number), in that iteration order.  See the module docstring for `method`, `dtype`,
  `eps_all`, the three parameters and the errors."""
  if method not in METHODS:
    raise ValueError('simulate: unknown method %r (%s)' % (method, ' '.join(METHODS)))
  dtype = tile_checks.check_float_dtype(dtype, 'simulate')
  num_paths = int(num_paths)
  if num_paths < 1:
    raise ValueError('simulate: num_paths = %d must be at least 1' % num_paths)
  products = [(ts, te, lamb) for ts_a, te, lamb in zip(ts_all, te_all, lamb_all) for ts in ts_a]
  if eps_all is not None and len(eps_all) != len(products):
    raise ValueError('simulate: eps_all holds %d arrays for %d products' % (len(eps_all), len(products)))
  # (the three parameters before the first date is divided by delta; lamb with its product)
  _, _, _, _, _, delta, f0, theta = _swaption.check_operands(dtype, (1, num_paths), 2, 0.0, delta, f0, theta, what='simulate')
  band = max(util.divup(num_paths, context.get().num_workers), 1)
  swaptions = []
  for i, (ts, te, lamb) in enumerate(products):
    steps, maturities = _grid(ts, te, delta)
    _, _, _, _, lamb, delta, f0, theta = _swaption.check_operands(dtype, (steps, num_paths), maturities, lamb, delta, f0,
                                                                  theta, what='simulate')
    eps = _draws(None if eps_all is None else eps_all[i], steps, num_paths, band, dtype)
    if method == 'fused':
      v = _fused(eps, steps, maturities, num_paths, band, lamb, dtype, delta, f0, theta)
    else:
      v = _expr(eps, steps, maturities, num_paths, lamb, dtype, delta, f0, theta)
    v = expr.lazify(v)
    # Save expected value in bps and std.
    me = expr.mean(v) * 10000
    st = expr.std(v) / expr.sqrt(num_paths) * 10000
    swaptions.append([me.optimized().evaluate(), st.optimized().evaluate()])
  return swaptions
