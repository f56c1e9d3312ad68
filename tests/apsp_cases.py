"""Inputs, the oracle and the yardstick of the shortest-path tests (NumPy and scipy; shared by tests/test_apsp_cases_cpu.py,
tests/test_apsp_gpu.py and tests/test_isomap_example.py; not a test file).

Oracle: scipy.sparse.csgraph.shortest_path (Dijkstra) in float64 on the stored weights, the diagonal left out (the
kernel ignores it); +inf where there is no path.

Bound (derived, not measured): a path has at most n - 1 edges, hence at most n - 2 rounded adds, whatever the order in
which its pieces were joined, and all terms are positive; a stored value is therefore within

    gamma = (n - 1) u / (1 - (n - 1) u),     u = 2^-24 (float32) | 2^-53 (float64)

(relative) of the exact length of its path, and rounding is monotone, so the smallest stored candidate is within gamma
of the exact shortest length.  float32 results are held to gamma against the float64 oracle, float64 results to
2 gamma, because the oracle rounds too.  Integer weights in 1 .. 64 make every path sum over n <= 200 vertices exact in
float32 (at most 199 * 64 < 2^24): such results equal the oracle bit for bit."""
import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def gamma(n, dtype):
  m = max(n - 1, 0) * U[np.dtype(dtype)]
  return m / (1.0 - m)


def bound(n, dtype):
  return gamma(n, dtype) * (2 if np.dtype(dtype) == np.float64 else 1)


def _rng(seed, n, degree):
  return np.random.RandomState(20150710 + 7919 * seed + 31 * n + 977 * degree)


def _directed(n, degree, rng, draw, diagonal):
  """A random directed graph as a dense matrix of float64: about 10 % of the vertices (one at least from n = 2 on) are
  isolated, every other vertex has `degree` edges to other connected vertices; `diagonal` is what the diagonal holds
  (it is ignored by the code under test)."""
  w = np.full((n, n), np.inf)
  if n >= 2:
    isolated = rng.permutation(n)[:max(1, n // 10)]
    live = np.setdiff1d(np.arange(n), isolated)
    for i in live:
      others = live[live != i]
      if others.size:
        to = rng.choice(others, size=min(degree, others.size), replace=False)
        w[i, to] = draw(to.size)
  np.fill_diagonal(w, diagonal)
  return w


def integer_graph(n, degree, dtype, seed=0):
  """Random directed graph, integer weights in 1 .. 64 (every path sum exact in float32 for n <= 200), 5 on the diagonal."""
  rng = _rng(seed, n, degree)
  return _directed(n, degree, rng, lambda m: rng.randint(1, 65, size=m).astype(np.float64), 5.0).astype(dtype)


def real_graph(n, degree, dtype, seed=0):
  """Random directed graph, weights uniform in [0.5, 2), 0 on the diagonal."""
  rng = _rng(seed + 1000, n, degree)
  return _directed(n, degree, rng, lambda m: rng.uniform(0.5, 2.0, size=m), 0.0).astype(dtype)


def permuted_chain(n, dtype, seed=0):
  """One undirected path through all n vertices, labels permuted at random, integer weights in 1 .. 64: the only route
  between its ends crosses every block of the matrix in scrambled order."""
  rng = _rng(seed + 2000, n, 1)
  w = np.full((n, n), np.inf)
  order = rng.permutation(n)
  for a, b in zip(order[:-1], order[1:]):
    w[a, b] = w[b, a] = float(rng.randint(1, 65))
  np.fill_diagonal(w, 0)
  return w.astype(dtype)


_oracles = {}


def oracle(w):
  """Shortest-path lengths of the stored weights in float64 (+inf: no path; 0 on the diagonal); computed once per input."""
  key = (w.tobytes(), w.shape, w.dtype.str)
  if key not in _oracles:
    if len(_oracles) > 64:
      _oracles.clear()
    n = w.shape[0]
    if n == 0:
      out = np.zeros((0, 0))
    else:
      from scipy.sparse import csr_matrix
      from scipy.sparse.csgraph import shortest_path
      w64 = w.astype(np.float64)
      edge = np.isfinite(w64) & ~np.eye(n, dtype=bool)
      i, j = np.nonzero(edge)
      out = shortest_path(csr_matrix((w64[edge], (i, j)), shape=(n, n)), method='D', directed=True)
    out.setflags(write=False)
    _oracles[key] = out
  return _oracles[key]


def check_exact(got, w):
  """Integer weights: the result equals the oracle bit for bit, +inf and the zero diagonal included."""
  assert got.dtype == w.dtype and got.shape == w.shape
  assert got.tobytes() == oracle(w).astype(w.dtype).tobytes()


def check_real(got, w, label='', limit=None):
  """Real weights: +inf exactly where the oracle has it, 0 on the diagonal, every other entry within the bound
  (relative).  Prints the fraction of the bound used before asserting."""
  want = oracle(w)
  n = w.shape[0]
  limit = bound(n, w.dtype) if limit is None else limit
  assert got.dtype == w.dtype and got.shape == w.shape
  assert np.array_equal(np.isposinf(got), np.isposinf(want))
  assert not np.any(np.diagonal(got))
  fin = np.isfinite(want) & (want > 0)
  err = np.abs(got[fin].astype(np.float64) - want[fin]) / want[fin]
  worst = float(err.max()) if err.size else 0.0
  print('apsp %s n=%d %s: max |got - oracle| / oracle = %.3g = %.3g of the bound %.3g'
        % (label, n, w.dtype.name, worst, worst / limit if limit else 0.0, limit))
  assert np.all(np.isfinite(got[fin]))
  assert worst <= limit
