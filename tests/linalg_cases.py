"""Inputs and yardsticks shared by tests/test_linalg_gpu.py and tests/test_cholesky_example.py.

Inputs: A = G . G^T + n I with G = RandomState(20150708).randn(n, n) cast to the dtype under test (the product taken in
float64 and stored in that dtype: the stored matrix IS the input), B the next randn(m, n) of the same stream.
Yardsticks: Higham's componentwise backward error bounds for the Cholesky factorisation (Accuracy and Stability of
Numerical Algorithms, 2nd ed., Theorem 10.3) and for substitution (Theorem 8.5), taken in the Frobenius norm, all
arithmetic of the check in float64 on the host:
    |A - L L^T|  <= gamma_{n+1} |L| |L^T|        |X L^T - B| <= gamma_n |X| |L^T|        gamma_k = k u / (1 - k u)
They hold for every order of summation and for the blocked forms, so they are bounds on ANY correct implementation in
that precision, not tuned numbers."""
import functools

import numpy as np

NB, OB, RB = 64, 256, 128          # csrc/linalg.hip: LDS block order, outer block order, rows per workgroup of the solve
ORDERS = (1, NB - 1, NB, NB + 1, OB - 1, OB, OB + 1, 3 * OB + 17)
ROWS = (1, 37, RB + 1)
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def gamma(k, dtype):
  ku = k * U[np.dtype(dtype)]
  return ku / (1 - ku)


@functools.lru_cache(maxsize=None)
def _drawn(n, m, dtype):
  rng = np.random.RandomState(20150708)
  g = rng.randn(n, n).astype(dtype).astype(np.float64)
  a = (g.dot(g.T) + n * np.eye(n)).astype(dtype)
  b = rng.randn(m, n).astype(dtype)
  a.setflags(write=False)
  b.setflags(write=False)
  return a, b


def spd(n, dtype):
  return _drawn(n, 37, np.dtype(dtype))[0]


def rhs(m, n, dtype):
  return _drawn(n, m, np.dtype(dtype))[1]


@functools.lru_cache(maxsize=None)
def factor(n, dtype):
  """A lower triangular L of the dtype under test for the solve's tests: LAPACK's factor of spd(n)."""
  low = np.linalg.cholesky(spd(n, dtype).astype(np.float64)).astype(dtype)
  low.setflags(write=False)
  return low


def fro(x):
  return float(np.sqrt((np.asarray(x, np.float64) ** 2).sum()))


def potrf_ratio(a, low):
  """||A - L L^T||_F / (gamma_{n+1} || |L| |L^T| ||_F): at most 1 for a backward stable factorisation."""
  n = a.shape[0]
  a64, l64 = np.tril(np.asarray(a, np.float64)), np.asarray(low, np.float64)
  resid = np.tril(l64.dot(l64.T)) - a64                  # the factorisation reads (and reproduces) the lower triangle
  resid = resid + np.tril(resid, -1).T
  return fro(resid) / (gamma(n + 1, a.dtype) * fro(np.abs(l64).dot(np.abs(l64.T))))


def trsm_ratio(b, low, x):
  n = low.shape[0]
  b64, l64, x64 = (np.asarray(v, np.float64) for v in (b, np.tril(low), x))
  return fro(x64.dot(l64.T) - b64) / (gamma(n, b.dtype) * fro(np.abs(x64).dot(np.abs(l64.T))))
