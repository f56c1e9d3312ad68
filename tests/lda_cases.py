"""Inputs, an oracle and a DERIVED error bound for the LDA (CVB0) step -- sp_lda_step and examples/_lda.step_numpy.
Pure NumPy; shared by the CPU and the GPU tests.

Oracle.  `oracle` follows the reference's order of operations (spartan/examples/lda.py:22-50: per document, per inner
iteration p = (N + eta) (gamma + alpha) / den, p / sum_t p, times x, the 1-norms, the normalisation; the last
iteration's q added to delta) in numpy.longdouble from the STORED operands: X and N as the dtype T holds them, alpha
and eta rounded to T once (that rounding is part of the kernel's contract, not of its error).  Its own error is some
thousand times below the float64 bound and is neglected.

Bound.  u = eps / 2 is the unit roundoff of T; every quantity below is a RELATIVE error to first order in u.  With
non-negative X and N every sum has non-negative terms, so a sum of n terms adds at most (n - 1) u in any order and a
product or a quotient adds u to the errors of its operands.  The form under test is A = (N + eta) / den, B = gamma +
alpha, s = sum_t a b, w = x / s, c = b . sum_j |a| |w|, gamma' = c / sum_t c:
    den = sum_j |N| + eta V    (V - 1) u for the sum, u for the product, u for the addition       (V + 1) u
    a   = (N + eta) / den      one addition, one quotient                                 eA  =  (V + 3) u
    b   = gamma + alpha        gamma carries g; an addition of positives                  eB  =  g + u
    s   = sum_t a b            a product, k terms                                                eA + eB + k u
    w   = x / s                                                                           eW  =  eA + eB + (k + 1) u
    c   = b sum_j a w          a product, at most V terms, a product           eC = 2 eA + 2 eB + (V + k + 2) u
    gamma' = c / sum_t c       k terms, a quotient                             g'  = 2 eC + k u
so one inner iteration takes g to
    g' = 4 g + (6 V + 3 k + 20) u :
it passes on four times the incoming error of gamma (twice through a b / s, and both doubled by the normalisation) and
adds the roundings of a k-term and a V-term sum plus a fixed handful of operations.  g_0 = u (the rounding of 1 / k),
and the bound on doc_topics is g_iters.  delta = a . sum_d w b with the B that entered the last iteration (error
g_{iters - 1}): a product, at most D terms, a product,
    eD = eA + u + (D - 1) u + (eW + eB + u) = 2 g_{iters - 1} + (2 V + k + D + 10) u,
whatever the ranges.  For signed X, c is unchanged (it sums |q|) and delta's terms keep the same relative errors each,
so the bound on delta is eD . sum_d |q|, which `oracle` returns as 'absq'.  The first-order figures are multiplied by
1.01 for the higher-order terms, which is ample while the bound is below 1e-2 (asserted).

The bound is derived, not fitted: the tests print the share of it that the code under test uses, and a share above one
half for step_numpy at any listed shape would mean that the derivation is wrong, not that the tolerance is tight."""
import functools

import numpy as np

L = np.longdouble
ALPHA, ETA = 0.1, 0.1


def case(v, d, k, dtype, seed=0, signed=False):
  """(X [v, d], N [k, v]) in `dtype`: counts from randint(0, 5) with about half the entries zeroed, document 7 empty
  (when there are more than 8), term 11 in no document (when there are more than 12), X[0, 0] = 3; N uniform in
  [0, 1).  signed: every third non-zero count negated."""
  rng = np.random.RandomState(1000 * seed + 7 * v + 3 * d + k)
  x = rng.randint(0, 5, size=(v, d)).astype(np.float64)
  x[rng.rand(v, d) < 0.5] = 0
  if v and d:
    x[0, 0] = 3
  if d > 8:
    x[:, 7] = 0
  if v > 12:
    x[11, :] = 0
  if signed:
    flat = x.reshape(-1)
    nzi = np.flatnonzero(flat)
    flat[nzi[::3]] *= -1
  n = rng.rand(k, v)
  return np.ascontiguousarray(x, dtype=dtype), np.ascontiguousarray(n, dtype=dtype)


def oracle(x, n, alpha, eta, iters):
  """dict(delta [k, V], absq [k, V] = sum_d |q|, doc_topics [D, k]) in longdouble, the reference's order of
  operations; alpha and eta rounded to the dtype of x once."""
  dt = x.dtype
  X, N = x.astype(L), n.astype(L)
  al, et = L(dt.type(alpha)), L(dt.type(eta))
  v, d = x.shape
  k = n.shape[0]
  den = np.abs(N).sum(axis=1) + et * v
  delta, absq, doc_topics = np.zeros((k, v), L), np.zeros((k, v), L), np.zeros((d, k), L)
  with np.errstate(all='ignore'):
    for doc in range(d):
      nzj = np.nonzero(X[:, doc])[0]
      gamma = np.ones(k, L) / k
      q = np.zeros((k, len(nzj)), L)
      for _ in range(iters):
        p = (N[:, nzj] + et) * (gamma + al)[:, None] / den[:, None]
        q = (p / p.sum(axis=0)[None, :]) * X[nzj, doc][None, :]
        c = np.abs(q).sum(axis=1)
        gamma = c / np.abs(c).sum()
      doc_topics[doc] = gamma
      delta[:, nzj] += q
      absq[:, nzj] += np.abs(q)
  return dict(delta=delta, absq=absq, doc_topics=doc_topics)


@functools.lru_cache(maxsize=None)
def oracle_of_case(v, d, k, dtype, iters, seed=0, signed=False):
  """The oracle of case(...) at ALPHA, ETA, computed once per process and left unchanged by its users."""
  x, n = case(v, d, k, np.dtype(dtype), seed=seed, signed=signed)
  out = oracle(x, n, ALPHA, ETA, iters)
  for a in out.values():
    a.setflags(write=False)
  return out


def eps(v, d, k, iters, dtype, nu=0.0):
  """dict(doc_topics=, delta=): the derived relative bounds (module docstring).  nu: the relative error that the
  entries of N carry already (driver_eps)."""
  u = float(np.finfo(dtype).eps) / 2
  g = prev = u
  for _ in range(iters):
    prev, g = g, 4 * g + (6 * v + 3 * k + 20) * u + 8 * nu
  out = dict(doc_topics=1.01 * g, delta=1.01 * (2 * prev + (2 * v + k + d + 10) * u + 4 * nu))
  assert max(out.values()) < 1e-2, out
  return out


def driver_eps(v, d_tile, k, iters, max_iter, tiles, dtype):
  """dict(doc_topics=, counts=): relative bounds on what learn_topics computes in `dtype` from a float64 start and
  small integer counts, against the exact chain.  If the entries of N (non-negative) carry a relative error nu, then
  N + eta and den carry at most nu and a = (N + eta) / den at most 2 nu beyond its own roundings; every term being
  positive, that is eA + 2 nu in the derivation of the module docstring: 8 nu more per inner iteration, 4 nu more in
  delta.  A training iteration forms N + delta per tile (an addition of positives: max(nu, eD) + u <= eD + u) and adds
  the `tiles` tiles ((tiles - 1) u), so nu' = eD(nu) + tiles . u, from nu_0 = u for the rounding of the start to
  float32 and 0 in float64.  The inference has eps(nu_max_iter)['doc_topics']; the normalised counts divide by a sum of
  V absolute values: 2 nu + V u."""
  u = float(np.finfo(dtype).eps) / 2
  nu = 0.0 if np.dtype(dtype) == np.dtype(np.float64) else u
  for _ in range(max_iter):
    nu = eps(v, d_tile, k, iters, dtype, nu=nu)['delta'] + tiles * u
  return dict(doc_topics=eps(v, d_tile, k, iters, dtype, nu=nu)['doc_topics'], counts=1.01 * (2 * nu + v * u))


def check_step(x, n, alpha, eta, iters, delta, doc_topics, want=None, label=''):
  """Assert delta and / or doc_topics (None: not given) against the oracle inside eps(); prints and returns the share
  of each bound that is used."""
  dt = x.dtype
  v, d = x.shape
  k = n.shape[0]
  want = want if want is not None else oracle(x, n, alpha, eta, iters)
  e = eps(v, d, k, iters, dt)
  share = {}
  if doc_topics is not None:
    assert doc_topics.dtype == dt and doc_topics.shape == (d, k)
    w = want['doc_topics']
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(doc_topics), nan), '%s: NaN rows differ' % label
    assert np.array_equal(nan.all(axis=1), nan.any(axis=1)) and np.array_equal(nan.all(axis=1), ~(x != 0).any(axis=0))
    err = np.abs(doc_topics.astype(L)[~nan] - w[~nan])
    lim = e['doc_topics'] * np.abs(w[~nan])
    share['doc_topics'] = float((err / lim).max()) if err.size else 0.0
  if delta is not None:
    assert delta.dtype == dt and delta.shape == (k, v)
    assert np.all(np.isfinite(delta)), '%s: delta is not finite' % label
    err = np.abs(delta.astype(L) - want['delta'])
    lim = e['delta'] * want['absq']
    assert not np.any(delta[want['absq'] == 0]), '%s: a term without a document has a non-zero delta' % label
    pos = lim > 0
    share['delta'] = float((err[pos] / lim[pos]).max()) if pos.any() else 0.0
  print('%s: share of the derived bound used: %s (bounds %s)'
        % (label, ', '.join('%s %.3g' % kv for kv in sorted(share.items())),
           ', '.join('%s %.3g' % kv for kv in sorted(e.items()))))
  for name, s in share.items():
    assert s <= 1.0, '%s: %s uses %.3g of its bound' % (label, name, s)
  return share


# ---------------------------------------------------------------- the input of tests/golden/lda_w4.npz
GOLDEN_V, GOLDEN_D, GOLDEN_K, GOLDEN_BANDS = 48, 40, 5, 4


def golden_input():
  """(X [48, 40] float64 counts, N0 [5, 48] float64): randint(0, 5) with about half the entries zeroed, document 7
  empty, term 11 in no document; N0 = rand(5, 48)."""
  rng = np.random.RandomState(20150708)
  x = rng.randint(0, 5, size=(GOLDEN_V, GOLDEN_D)).astype(np.float64)
  x[rng.rand(GOLDEN_V, GOLDEN_D) < 0.5] = 0
  x[:, 7] = 0
  x[11, :] = 0
  return x, rng.rand(GOLDEN_K, GOLDEN_V)
