"""Inputs, the oracle and the yardsticks of the nearest-neighbour tests (pure NumPy; shared by tests/test_knn_gpu.py and
tests/test_neighbors_example.py).

Oracle: the squared distances in the DIFFERENCE form sum_j (q_j - x_j)^2, every term and the sum in extended precision
(numpy.longdouble: never less than float64, 64 significand bits where the host has them, so that the oracle's own
error stays below the float64 kernels'), and numpy.lexsort on (index, d2) for the order: ascending distance, equal
distances by ascending index.  A point whose distance is NaN is no neighbour; missing neighbours are +inf / -1.

Bound (derived, not measured): a computed d2 is a sum of d non-negative terms, each from one rounded subtract and one
rounded multiply, joined by at most d - 1 rounded adds; every term therefore carries at most d + 1 factors (1 + delta),
|delta| <= u, in ANY summation order, and |computed - exact| <= gamma * exact with

    gamma = (d + 2) u / (1 - (d + 2) u),     u = 2^-24 (float32) | 2^-53 (float64)

(Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1; d + 2 leaves one factor of margin).  Consequence
for the ORDER: if the kernel returns index j at position i, then at least i + 1 points have a computed distance <= that
of j and at most i points a smaller one, hence for e = exact d2 of j and s = the exact i-th smallest distance

    (1 - gamma) / (1 + gamma) * s  <=  e  <=  (1 + gamma) / (1 - gamma) * s.
"""
import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
NO_INDEX = np.iinfo(np.int64).max
BIG_OFFSET = 2 ** 33 + 5


def gamma(d, dtype):
  n = (d + 2) * U[np.dtype(dtype)]
  return n / (1.0 - n)


def integer_case(nq, npts, d, dtype, seed=0):
  """(q, x) with small integer coordinates -- [-2, 2] up to d = 4, [-8, 8] above: every squared distance is an integer
  below 2^24 (d <= 200: at most 200 * 16^2), exact in float32 in any summation order, and equal distances abound."""
  rng = np.random.RandomState(20150708 + 7919 * seed + nq + 31 * npts + 977 * d)
  lim = 2 if d <= 4 else 8
  q = rng.randint(-lim, lim + 1, size=(nq, d)).astype(dtype)
  x = rng.randint(-lim, lim + 1, size=(npts, d)).astype(dtype)
  return q, x


CLUSTER = 20


def real_case(nq, npts, d, dtype, seed=0):
  """(q, x): standard normal coordinates; twenty points of x, spread over its rows, lie within 1e-3 of one another, and
  the first five queries lie beside that cluster, so that their nearest neighbours are all but equidistant."""
  rng = np.random.RandomState(20150709 + 7919 * seed + nq + 31 * npts + 977 * d)
  q = rng.randn(nq, d)
  x = rng.randn(npts, d)
  centre = rng.randn(d)
  rows = np.linspace(0, npts - 1, min(CLUSTER, npts)).astype(np.int64)
  x[rows] = centre + rng.uniform(-1, 1, size=(rows.size, d)) * (0.5e-3 / np.sqrt(d))
  q[:min(5, nq)] = centre + rng.randn(min(5, nq), d) * 0.05
  return q.astype(dtype), x.astype(dtype)


def exact_dist2(q, x):
  """[nq, np] squared distances of the stored values, difference form, in extended precision."""
  ql, xl = q.astype(np.longdouble), x.astype(np.longdouble)
  out = np.zeros((q.shape[0], x.shape[0]), np.longdouble)
  with np.errstate(all='ignore'):
    for j in range(q.shape[1]):
      diff = ql[:, j, None] - xl[None, :, j]
      out += diff * diff
  return out


def select(d2, idx, valid, k):
  """Per row the k smallest candidates by (d2, idx) among the valid ones: (d2 [nq, k], idx int64 [nq, k]), padded
  with +inf / -1."""
  nq, m = d2.shape
  d2 = np.where(valid, d2, np.inf)
  idx = np.where(valid, idx, NO_INDEX).astype(np.int64)
  if m < k:
    d2 = np.concatenate([d2, np.full((nq, k - m), np.inf, d2.dtype)], axis=1)
    idx = np.concatenate([idx, np.full((nq, k - m), NO_INDEX, np.int64)], axis=1)
  order = np.lexsort((idx, d2), axis=1)[:, :k]
  out_d, out_i = np.take_along_axis(d2, order, axis=1), np.take_along_axis(idx, order, axis=1)
  out_i[out_i == NO_INDEX] = -1
  return out_d, out_i


_oracles = {}


def oracle(q, x, k, index_offset=0):
  """(d2 in extended precision [nq, k], idx int64 [nq, k]) of the exact search; computed once per input."""
  key = (q.tobytes(), x.tobytes(), q.shape, x.shape, q.dtype.str, int(k), int(index_offset))
  if key not in _oracles:
    if len(_oracles) > 64:
      _oracles.clear()
    d2 = exact_dist2(q, x)
    idx = np.broadcast_to(np.arange(x.shape[0], dtype=np.int64) + int(index_offset), d2.shape)
    out = select(d2, idx, ~np.isnan(d2), k)
    for a in out:
      a.setflags(write=False)
    _oracles[key] = out
  return _oracles[key]


def check_exact(dist2, idx, q, x, k, index_offset=0):
  """Integer-valued inputs: both outputs equal the oracle bit for bit, ties and padding included."""
  want_d, want_i = oracle(q, x, k, index_offset)
  assert dist2.dtype == q.dtype and idx.dtype == np.int64
  assert dist2.shape == (q.shape[0], k) and idx.shape == (q.shape[0], k)
  np.testing.assert_array_equal(idx, want_i)
  assert dist2.tobytes() == want_d.astype(q.dtype).tobytes()


def check_real(dist2, idx, q, x, k, index_offset=0, d2_dtype=None, label=''):
  """Real-valued inputs (np >= k): the four properties of the module docstring, for every query and every position.
  dist2: what the code under test returned as squared distances (any float dtype); the bound is the one of
  `d2_dtype` (default: the inputs' dtype).  Prints the worst figures, as fractions of their bounds, before asserting."""
  nq, npts = q.shape[0], x.shape[0]
  assert dist2.shape == (nq, k) and idx.shape == (nq, k) and idx.dtype == np.int64 and npts >= k
  g = gamma(q.shape[1], d2_dtype or q.dtype)
  exact = exact_dist2(q, x)
  local = idx - int(index_offset)
  assert np.all((local >= 0) & (local < npts)), 'indices out of range'
  assert all(np.unique(row).size == k for row in local), 'an index is returned twice'
  e = np.take_along_axis(exact, local, axis=1)
  s = np.sort(exact, axis=1)[:, :k]
  got = dist2.astype(np.longdouble)
  err = np.abs(got - e) / np.where(e > 0, g * e, 1)
  lo, hi = (1 - g) / (1 + g) * s, (1 + g) / (1 - g) * s
  spread = np.abs(e - s) / np.where(s > 0, (hi - s), 1)
  print('knn %s %dx%dx%d k=%d %s: max |dist2 - e| / (gamma e) = %.3g, max |e - s| / ((1+g)/(1-g) s - s) = %.3g'
        % (label, nq, npts, q.shape[1], k, q.dtype.name, float(err.max()), float(spread.max())))
  assert np.all(np.abs(got - e) <= g * e)
  assert np.all((lo <= e) & (e <= hi))
  d = np.diff(got, axis=1)
  assert np.all(d >= 0), 'distances decrease along a row'
  assert np.all((d > 0) | (np.diff(idx, axis=1) > 0)), 'equal distances are not in ascending index order'
