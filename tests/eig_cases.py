"""Inputs and yardsticks shared by tests/test_eig_gpu.py and tests/test_ssvd_example.py.

Inputs, from RandomState(20150708), built in float64 and stored in the dtype under test (the stored matrix IS the
input; the solver reads its lower triangle, so the checks take the symmetric matrix that triangle defines):
    indef       (G + G^T) / 2
    gram        B . B^T, B of shape n x 2n
    pm          Q diag(+-(1 + i // 2)) Q^T: pairs lambda, -lambda of equal magnitude (a one-sided Jacobi method mixes
                their eigenspaces)
    clustered   Q diag(1 ... 1, 2 ... 2) Q^T
Ratios, all arithmetic of the check in float64 on the host, u = 2^-24 | 2^-53:
    resid = ||A V - V diag(w)||_F / (n u ||A||_F)     orth = ||V^T V - I||_F / (n u)
    eigs  = max |w - eigvalsh(A)| / (n u ||A||_2)
The yardstick is `jacobi`, a NumPy transcription of the scheme sp_syevj states (csrc/linalg.hip): cyclic two-sided
Jacobi in the dtype under test, the pairs of round r of the round-robin tournament rotated together, Rutishauser's
formulas, stop at off(A)_F <= n u ||A||_F, at most 64 sweeps.  It applies each round as the plain products (A J, then
J^T (A J), V J), with none of the kernel's refinements, and is not the code under test.  A device result may exceed
the transcription's ratio on the same input by the factor MARGIN = 4 (fused or re-associated products, the explicit
zero, a threshold for tiny rotations: a small constant each); LAPACK's own ratios (0.001 to 1.7) are no usable bound,
Jacobi's loss of orthogonality grows like sweeps . n^1.5 . u.

The transcription takes 2 to 9 s per input at n = 257, so its ratios on the inputs of tests/test_eig_gpu.py are kept in
tests/golden/eig_yardstick.json (written by tests/golden/make_golden_eig.py from `jacobi` below, nothing else);
tests/test_eig_cases_cpu.py runs the transcription itself on the small orders and compares."""
import functools
import json
import os

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
KINDS = ('indef', 'gram', 'pm', 'clustered')
MAX_SWEEPS = 64
MARGIN = 4.0
LDS_ORDER = {np.dtype(np.float32): 64, np.dtype(np.float64): 63}     # csrc/linalg.hip: SyevjLds<T>::N


@functools.lru_cache(maxsize=None)
def _matrix(kind, n, dtype):
  rng = np.random.RandomState(20150708)
  if kind == 'indef':
    g = rng.randn(n, n)
    a = (g + g.T) / 2
  elif kind == 'gram':
    b = rng.randn(n, 2 * n)
    a = b.dot(b.T)
  else:
    q = np.linalg.qr(rng.randn(n, n))[0]
    i = np.arange(n)
    lam = (1.0 + i // 2) * np.where(i % 2, -1.0, 1.0) if kind == 'pm' else np.where(i < n // 2, 1.0, 2.0)
    a = (q * lam).dot(q.T)
    a = (a + a.T) / 2
  a = a.astype(dtype)
  a.setflags(write=False)
  return a


def matrix(kind, n, dtype):
  assert kind in KINDS
  return _matrix(kind, int(n), np.dtype(dtype))


def symmetric64(a):
  """The float64 symmetric matrix the lower triangle of `a` defines."""
  low = np.tril(np.asarray(a, np.float64))
  return low + np.tril(low, -1).T


def fro(x):
  return float(np.sqrt((np.asarray(x, np.float64) ** 2).sum()))


def ratios(a, w, v):
  """(resid, orth, eigs) of the computed pair (w, v) for the input `a` (whose dtype sets u)."""
  n = a.shape[0]
  nu = n * U[np.dtype(a.dtype)]
  a64, w64, v64 = symmetric64(a), np.asarray(w, np.float64), np.asarray(v, np.float64)
  if n == 0:
    return 0.0, 0.0, 0.0
  norm_f, norm_2 = fro(a64), float(np.abs(np.linalg.eigvalsh(a64)).max())
  resid = fro(a64.dot(v64) - v64 * w64) / (nu * norm_f) if norm_f else 0.0
  orth = fro(v64.T.dot(v64) - np.eye(n)) / nu
  eigs = float(np.abs(w64 - np.linalg.eigvalsh(a64)).max()) / (nu * norm_2) if norm_2 else 0.0
  return resid, orth, eigs


def round_pairs(n, r):
  """The pairs (p < q) of round r of the tournament on n indices (n - 1 rounds for even n, n for odd n, where the
  index paired with the missing one sits out): index m - 1 meets r, every other i meets i' with i + i' = 2 r mod m - 1."""
  m = n + (n & 1)
  k = np.arange(1, m // 2)
  x, y = (r + k) % (m - 1), (r - k) % (m - 1)
  p, q = np.minimum(x, y), np.maximum(x, y)
  if m - 1 < n:
    p, q = np.concatenate(([r], p)), np.concatenate(([m - 1], q))
  return p, q


def jacobi(a, max_sweeps=MAX_SWEEPS):
  """(w ascending, V, info, sweeps): the transcription, in a.dtype."""
  dt = a.dtype
  n = a.shape[0]
  low = np.tril(a)
  A = (low + np.tril(low, -1).T).astype(dt)
  Vt = np.eye(n, dtype=dt)                # V^T
  m = n + (n & 1)
  nu = n * U[np.dtype(dt)]
  one = dt.type(1)
  sweeps = 0
  while True:
    a64 = A.astype(np.float64)
    off, norm = fro(a64 - np.diag(np.diag(a64))), fro(a64)
    if off <= nu * norm:
      info = 0
      break
    if sweeps == max_sweeps:
      info = 1
      break
    for r in range(m - 1):
      p, q = round_pairs(n, r)
      app, aqq, apq = A[p, p], A[q, q], A[q, p]
      with np.errstate(all='ignore'):
        tau = (aqq - app) / (2 * apq)
        t = np.copysign(one, tau) / (np.abs(tau) + np.sqrt(one + tau * tau))
        c = one / np.sqrt(one + t * t)
        s = t * c
      skip = (apq == 0) | ~np.isfinite(tau)
      c, s = np.where(skip, one, c).astype(dt), np.where(skip, 0, s).astype(dt)
      cc, ss = c[:, None], s[:, None]
      # A J: its columns p, q are the rows p, q of (A J)^T = J^T A^T -- the same products, taken on contiguous rows
      T = np.ascontiguousarray(A.T)
      Tp, Tq = T[p], T[q]
      T[p], T[q] = cc * Tp - ss * Tq, ss * Tp + cc * Tq
      A = np.ascontiguousarray(T.T)
      Ap, Aq = A[p], A[q]
      A[p], A[q] = cc * Ap - ss * Aq, ss * Ap + cc * Aq            # J^T (A J)
      Vp, Vq = Vt[p], Vt[q]
      Vt[p], Vt[q] = cc * Vp - ss * Vq, ss * Vp + cc * Vq          # (V J)^T
    sweeps += 1
  d = np.diag(A).copy()
  order = np.argsort(d, kind='stable')
  return d[order], np.ascontiguousarray(Vt[order].T), info, sweeps


@functools.lru_cache(maxsize=None)
def _yardstick(kind, n, dtype):
  a = _matrix(kind, n, dtype)
  w, v, info, sweeps = jacobi(a)
  assert info == 0
  return ratios(a, w, v) + (sweeps,)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'eig_yardstick.json')


def key(kind, n, dtype):
  return '%s-%d-%s' % (kind, n, np.dtype(dtype).name)


@functools.lru_cache(maxsize=None)
def recorded():
  with open(GOLDEN) as f:
    return json.load(f)


def yardstick(kind, n, dtype, live=False):
  """(resid, orth, eigs, sweeps) of the transcription on matrix(kind, n, dtype): the recorded run, or (live, or
  nothing recorded for this input) a run made now, once."""
  rec = None if live else recorded().get(key(kind, n, dtype))
  if rec is not None:
    return tuple(rec)
  return _yardstick(kind, int(n), np.dtype(dtype))


def check(label, a, w, v, yard):
  """Prints every ratio of (w, v) next to its limit, MARGIN x the transcription's `yard`, then asserts them."""
  got = ratios(a, w, v)
  ok = True
  for name, g, y in zip(('resid', 'orth', 'eigs'), got, yard[:3]):
    print('%s: %s = %.4g  limit %.4g (transcription %.4g)' % (label, name, g, MARGIN * y, y))
    ok = ok and g <= MARGIN * y
  assert ok, (label, got, yard)
  return got
