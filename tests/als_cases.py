"""Inputs, oracle and error bound of the ALS half-step (sp_als_solve, examples/_als.py).  Pure NumPy.

Oracle.  For row i, A_i and b_i as include/spartan_hip_als.h states them, formed in numpy.longdouble from the stored
operands (la and alpha rounded to the operands' dtype once, as the kernel takes them); A_i x = b_i solved in float64
with one step of refinement on the longdouble residual.

Bound (derived, not measured).  u = 2^-24 or 2^-53, gamma_k = k u / (1 - k u).  Every entry of the computed A_i is a
sum of t products, each with at most three more roundings (the weight, the product, the diagonal term): Higham, Accuracy
and Stability of Numerical Algorithms, Lemma 3.1 gives |dA| <= gamma_{t+3} |Y|^T |W_i| |Y| (+ |Y|^T |Y| in implicit
mode), with t = n terms in explicit mode and 2 n in implicit mode (the rated items and Y^T Y).  The Cholesky solve adds
|dA| <= gamma_{3f+1} |L| |L|^T (Theorem 10.4), in norm at most f gamma_{3f+1} ||A_i||_2.  b_i: gamma_{n+2} |Y|^T |c_i|.
The normwise perturbation theorem 7.2 then gives

  eA = (gamma_{t+3} || |Y|^T |W_i| |Y| (+ |Y|^T |Y|) ||_2 + f gamma_{3f+1} ||A_i||_2) / ||A_i||_2
  eb = gamma_{n+2} || |Y|^T |c_i| ||_2 / ||b_i||_2
  ||x^ - x||_2 / ||x||_2 <= kappa_2(A_i) (eA + eb) / (1 - kappa_2(A_i) eA)

and a case with kappa eA >= 1 is rejected (none of the cases here is).  At large n the float32 bound is loose (about
1e-2 at n = 2049): it is the float64 run of the same case, bounded near 1e-11, that catches a dropped or doubled term;
the float32 run checks the float32 instantiation.

Cases.  Ratings are integers in 0 .. 4 (80 % rated), factors uniform in [0, 1); row 1 is all zero and row 2 has a single
rating; a variant has negative ratings (explicit mode only: they make an implicit system indefinite -- the failure
path).  la = 0.065, alpha = 40: the driver's defaults.
"""
import functools

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
LA, ALPHA = 0.065, 40.0
LD = np.longdouble


def gamma(k, dtype):
  ku = k * U[np.dtype(dtype)]
  assert ku < 1
  return ku / (1 - ku)


@functools.lru_cache(maxsize=None)
def case(m, n, f, dtype, seed=0, negative=False):
  """(ratings [m, n], factors [n, f]) in `dtype`, read-only."""
  rng = np.random.RandomState(20150713 + 7919 * seed + 31 * m + 17 * n + f)
  r = rng.randint(-2 if negative else 0, 5, size=(m, n)).astype(dtype)
  if m > 1:
    r[1] = 0
  if m > 2 and n > 0:
    r[2] = 0
    r[2, n // 2] = 3
  y = rng.rand(n, f).astype(dtype)
  r.setflags(write=False)
  y.setflags(write=False)
  return r, y


def _norm2(a):
  a = np.asarray(a, np.float64)
  return float(np.linalg.norm(a, 2)) if a.size else 0.0


def systems(r, y, la=LA, alpha=ALPHA, implicit=False):
  """Per row (A, b, absA, absb, rated): the exact system and the matrices of absolute values the bound needs, all in
  longdouble."""
  dt = np.dtype(r.dtype)
  la, alpha = LD(dt.type(la)), LD(dt.type(alpha))
  rl, yl = np.asarray(r, LD), np.asarray(y, LD)
  f = y.shape[1]
  eye = np.eye(f, dtype=LD)
  gram = yl.T.dot(yl) if implicit else None
  agram = np.abs(yl).T.dot(np.abs(yl)) if implicit else None
  out = []
  for i in range(r.shape[0]):
    rated = ~(rl[i] == 0)
    ri, ys = rl[i][rated], yl[rated]
    if implicit:
      w = alpha * ri
      c = np.where(ri > 0, 1 + alpha * ri, LD(0))
      a = gram + (ys.T * w).dot(ys) + la * eye
      absa = agram + (np.abs(ys).T * np.abs(w)).dot(np.abs(ys))
    else:
      c = ri
      a = ys.T.dot(ys) + la * LD(ri.size) * eye
      absa = np.abs(ys).T.dot(np.abs(ys))
    out.append((a, ys.T.dot(c), absa, np.abs(ys).T.dot(np.abs(c)), int(ri.size)))
  return out


def _solve(a, b):
  a64 = np.asarray(a, np.float64)
  x = np.linalg.solve(a64, np.asarray(b, np.float64))
  resid = b - a.dot(np.asarray(x, LD))
  return x + np.linalg.solve(a64, np.asarray(resid, np.float64))


@functools.lru_cache(maxsize=None)
def _oracle_cached(m, n, f, dtype, seed, negative, la, alpha, implicit):
  r, y = case(m, n, f, dtype, seed, negative)
  return oracle(r, y, la, alpha, implicit)


def oracle(r, y, la=LA, alpha=ALPHA, implicit=False):
  """(x [m, f] float64, bound [m], kappa [m]): the solution of every row and the derived bound on the relative 2-norm
  error of a computation in the dtype of r; a row whose solution is exactly 0 (nothing rated; b_i = 0) has bound 0."""
  dt = np.dtype(r.dtype)
  m, n = r.shape
  f = y.shape[1]
  t = 2 * n if implicit else n
  x = np.zeros((m, f))
  bound, kappa = np.zeros(m), np.zeros(m)
  for i, (a, b, absa, absb, rated) in enumerate(systems(r, y, la, alpha, implicit)):
    if (not implicit and rated == 0) or not np.any(b):
      continue
    x[i] = _solve(a, b)
    na = _norm2(a)
    kappa[i] = np.linalg.cond(np.asarray(a, np.float64), 2)
    ea = (gamma(t + 3, dt) * _norm2(absa) + f * gamma(3 * f + 1, dt) * na) / na
    eb = gamma(n + 2, dt) * float(np.linalg.norm(np.asarray(absb, np.float64))) / float(np.linalg.norm(np.asarray(b, np.float64)))
    assert kappa[i] * ea < 1, 'the bound is void: kappa eA = %g' % (kappa[i] * ea)
    bound[i] = kappa[i] * (ea + eb) / (1 - kappa[i] * ea)
  return x, bound, kappa


def oracle_of_case(m, n, f, dtype, implicit, seed=0, negative=False, la=LA, alpha=ALPHA):
  """oracle(*case(...)), computed once per process."""
  return _oracle_cached(m, n, f, np.dtype(dtype), seed, negative, la, alpha, bool(implicit))


def errors(got, want):
  """Per row ||got - want||_2 / ||want||_2 (0 where both are exactly 0, inf where only `want` is)."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  num, den = np.linalg.norm(got - want, axis=1), np.linalg.norm(want, axis=1)
  with np.errstate(all='ignore'):
    return np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num > 0, np.inf, 0.0))


def check(got, want, bound, label='', scale=1.0):
  """Every row of `got` within scale x its bound of the oracle's row; rows whose bound is 0 are exactly 0.  Prints the
  measured figures first.  Returns the largest error / bound."""
  got = np.asarray(got)
  assert got.shape == want.shape, (got.shape, want.shape)
  err = errors(got, want)
  exact = bound == 0
  assert not np.any(got[exact]), '%s: a row that must be exactly 0 is not' % label
  ratio = float((err[~exact] / (scale * bound[~exact])).max()) if np.any(~exact) else 0.0
  print('%s: max relative error %.3g = %.3g of the bound (largest bound %.3g)'
        % (label, float(err[~exact].max()) if np.any(~exact) else 0.0, ratio, float(bound.max()) if bound.size else 0.0))
  assert np.all(err[~exact] <= scale * bound[~exact]), (label, err, bound)
  return ratio
