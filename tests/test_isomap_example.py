"""examples/sklearn/manifold: the Isomap driver.  CPU leg: the host framework on the injected NumPy backend, where the
graph bodies are the NumPy helpers beside the driver (examples/sklearn/manifold/_graph.py).  GPU leg: the same driver
on the HIP backend (sp_knn, sp_graph_from_knn, sp_apsp, the map and reduce kernels, sp_syevj).

Input: an S-curve of 200 points in 3-D, n_neighbors = 8.  Yardstick: scikit-learn's own Isomap(n_neighbors=8,
n_components=2, eigen_solver='dense') in float64 on the stored points.  For the seed used the neighbour graph is
connected and every row's 8th and 9th squared neighbour distances are more than 4 gamma_knn apart (relative), so the
edge set is the only right one (both asserted below).

dist_matrix_: a path of at most n - 1 edges, each edge sqrt(d2) with d2 within gamma_knn (tests/knn_cases.py, d = 3; the
half of it the square root leaves, plus the root's own rounding, stays below gamma_knn), joined within gamma_apsp
(tests/apsp_cases.py): (1 + gamma_apsp)(1 + gamma_knn) - 1, doubled in float64 because the yardstick rounds too.
embedding_: column by column after aligning signs, relative 2-norm error against scikit-learn's; the limit is
max(8 x the error of the plain recipe, n u), the recipe being the same steps in NumPy (numpy.linalg.eigh) in the dtype
under test -- the rule of tests/test_ssvd_example.py.  Measured figures are printed before each assertion."""
import functools
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples.sklearn.manifold import Isomap
from tests import apsp_cases as ac
from tests import knn_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))
N, K, SEED, MARGIN = 200, 8, 20150711, 8


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


@functools.lru_cache(maxsize=None)
def s_curve(dtype):
  rng = np.random.RandomState(SEED)
  t = 3 * np.pi * (rng.rand(N) - 0.5)
  x = np.stack([np.sin(t), 2.0 * rng.rand(N), np.sign(t) * (np.cos(t) - 1)], axis=1).astype(dtype)
  x.setflags(write=False)
  return x


@functools.lru_cache(maxsize=None)
def _neighbours(dtype):
  """(d2 [n, n] exact squared distances of the stored points without the diagonal, sorted order per row)."""
  x = s_curve(dtype)
  d2 = np.array(kc.exact_dist2(x, x))
  np.fill_diagonal(d2, np.inf)
  return d2, np.argsort(d2, axis=1, kind='stable')


@functools.lru_cache(maxsize=None)
def _sklearn(dtype):
  from sklearn.manifold import Isomap as SkIsomap
  sk = SkIsomap(n_neighbors=K, n_components=2, eigen_solver='dense').fit(s_curve(dtype).astype(np.float64))
  out = np.asarray(sk.dist_matrix_, np.float64), np.asarray(sk.embedding_, np.float64)
  for a in out:
    a.setflags(write=False)
  return out


def _dist_bound(dtype):
  b = (1 + ac.gamma(N, dtype)) * (1 + kc.gamma(3, dtype)) - 1
  return b * (2 if np.dtype(dtype) == np.float64 else 1)


def _column_errors(got, want):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  signs = np.sign((got * want).sum(axis=0))
  return np.linalg.norm(got * signs - want, axis=0) / np.linalg.norm(want, axis=0)


@functools.lru_cache(maxsize=None)
def _recipe_errors(dtype):
  """The plain recipe in NumPy in the dtype under test: brute-force neighbours, Floyd-Warshall, -0.5 D^2 double
  centred, numpy.linalg.eigh, V sqrt(w)."""
  x = s_curve(dtype)
  d2 = np.zeros((N, N), x.dtype)
  for j in range(x.shape[1]):
    diff = x[:, j, None] - x[None, :, j]
    d2 = d2 + diff * diff
  np.fill_diagonal(d2, np.inf)
  nearest = np.argsort(d2, axis=1, kind='stable')[:, :K]
  w = np.full((N, N), np.inf, x.dtype)
  rows = np.arange(N)[:, None]
  w[rows, nearest] = np.sqrt(np.take_along_axis(d2, nearest, axis=1))
  w = np.minimum(w, w.T)
  np.fill_diagonal(w, 0)
  for k in range(N):
    np.minimum(w, w[:, k, None] + w[None, k, :], out=w)
  g = w * w * x.dtype.type(-0.5)
  g = g - g.mean(axis=1, keepdims=True) - g.mean(axis=0, keepdims=True) + g.mean()
  lam, vecs = np.linalg.eigh(g)
  emb = vecs[:, ::-1][:, :2] * np.sqrt(lam[::-1][:2])
  assert emb.dtype == x.dtype
  return _column_errors(emb, _sklearn(dtype)[1])


def _fit(backend, workers, x, **kw):
  _start(backend, workers)
  try:
    return Isomap(**kw).fit(sp.from_numpy(x) if kw.pop('as_expr', True) else x)
  finally:
    sp.shutdown()


def _check(backend, workers, dtype):
  dtype = np.dtype(dtype)
  x = s_curve(dtype)
  iso = _fit(backend, workers, x, n_neighbors=K, n_components=2)
  sk_dist, sk_emb = _sklearn(dtype)
  dist, emb = iso.dist_matrix_, iso.embedding_
  assert isinstance(dist, np.ndarray) and dist.shape == (N, N) and dist.dtype == dtype
  assert isinstance(emb, np.ndarray) and emb.shape == (N, 2) and emb.dtype == dtype
  assert iso.nbrs_.n_neighbors == K and tuple(iso.training_data_.shape) == (N, 3)
  assert np.all(sk_dist[~np.eye(N, dtype=bool)] > 0) and not np.any(np.diagonal(dist))
  limit = _dist_bound(dtype)
  off = ~np.eye(N, dtype=bool)
  rel = np.abs(dist[off].astype(np.float64) - sk_dist[off]) / sk_dist[off]
  print('isomap %s w=%d %s: max |dist_matrix_ - sklearn| / sklearn = %.3g = %.3g of the bound %.3g'
        % (backend, workers, dtype.name, rel.max(), rel.max() / limit, limit))
  assert rel.max() <= limit
  assert dist.tobytes() == np.ascontiguousarray(dist.T).tobytes()
  got, yard = _column_errors(emb, sk_emb), _recipe_errors(dtype)
  floor = N * ac.U[dtype]
  ok = True
  for j in range(2):
    lim = max(MARGIN * yard[j], floor)
    print('isomap %s w=%d %s: error of embedding_ column %d = %.4g  limit %.4g (recipe %.4g, n u %.4g)'
          % (backend, workers, dtype.name, j, got[j], lim, yard[j], floor))
    ok = ok and got[j] <= lim
  assert ok, (got, yard)
  return iso


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_the_input_has_one_right_edge_set(dtype):
  d2, order = _neighbours(dtype)
  s = np.take_along_axis(d2, order, axis=1)
  gap = (s[:, K] - s[:, K - 1]) / s[:, K]
  g = kc.gamma(3, dtype)
  print('s-curve %s: smallest relative gap between the 8th and 9th squared neighbour distance = %.3g (4 gamma = %.3g)'
        % (np.dtype(dtype).name, gap.min(), 4 * g))
  assert gap.min() > 4 * g
  from scipy.sparse.csgraph import connected_components
  adj = np.zeros((N, N), bool)
  adj[np.arange(N)[:, None], order[:, :K]] = True
  assert connected_components(adj | adj.T, directed=False)[0] == 1


@pytest.mark.parametrize('workers', (1, 4))
def test_matches_scikit_learn_cpu(workers):
  _check('numpy', workers, np.float64)


def test_float32_and_numpy_input_cpu():
  _check('numpy', 4, np.float32)
  x = s_curve(np.float64)
  _start('numpy', 2)
  try:
    iso = Isomap(n_neighbors=K).fit(np.array(x))
    only = Isomap(n_neighbors=K).fit(np.array(x), embed=False)
  finally:
    sp.shutdown()
  assert iso.embedding_.shape == (N, 2) and not hasattr(only, 'embedding_')
  assert only.dist_matrix_.tobytes() == iso.dist_matrix_.tobytes()


def _two_clusters(dtype):
  rng = np.random.RandomState(SEED + 1)
  x = rng.rand(60, 3)
  x[30:] += 100.0
  return x.astype(dtype)


def _check_disconnected(backend, dtype):
  iso = _fit(backend, 2, _two_clusters(dtype), n_neighbors=5)
  d = iso.dist_matrix_
  assert not np.any(d[:30, 30:]) and not np.any(d[30:, :30])
  inside = ~np.eye(30, dtype=bool)
  assert np.all(d[:30, :30][inside] > 0) and np.all(d[30:, 30:][inside] > 0) and np.all(np.isfinite(d))
  assert iso.embedding_.shape == (60, 2) and np.all(np.isfinite(iso.embedding_))


def test_a_disconnected_graph_leaves_zeros_cpu():
  _check_disconnected('numpy', np.float64)


def test_duplicate_points_cpu():
  """Twelve copies of one point: the row itself is pushed out of its own list of 9, and the last entry goes instead."""
  x = np.array(s_curve(np.float64)[:60])
  x[:12] = x[0]
  iso = _fit('numpy', 1, x, n_neighbors=K)
  assert not np.any(iso.dist_matrix_[:12, :12]) and np.all(np.isfinite(iso.embedding_))


def test_refusals_cpu():
  x = np.array(s_curve(np.float64))
  with pytest.raises(NotImplementedError, match='dense'):
    _fit('numpy', 1, x, n_neighbors=K, eigen_solver='arpack')
  with pytest.raises(ValueError, match='127'):
    _fit('numpy', 1, x, n_neighbors=128)
  with pytest.raises(ValueError):
    _fit('numpy', 1, x, n_neighbors=K, eigen_solver='quantum')
  iso = Isomap()
  assert (iso.n_neighbors, iso.n_components, iso.eigen_solver, iso.tol, iso.max_iter, iso.neighbors_algorithm) == \
      (5, 2, 'auto', 0, None, 'auto')
  _fit('numpy', 1, x, n_neighbors=K, eigen_solver='dense', tol=1e-3, max_iter=7)       # accepted and unused


def _check_golden(backend):
  """The reference's own graph_shortest_path (Cython Dijkstra, undirected) on this test's neighbour graph, recorded by
  tests/golden/make_golden_isomap.py at 4 workers: dist_matrix_ within the same bound."""
  gold = np.load(os.path.join(HERE, 'golden', 'isomap_w4.npz'))
  x = s_curve(np.float64)
  assert gold['x'].tobytes() == x.tobytes()
  iso = _fit(backend, 4, x, n_neighbors=K)
  ref = gold['dist_matrix']
  off = ~np.eye(N, dtype=bool)
  assert np.all(ref[off] > 0)
  rel = np.abs(iso.dist_matrix_[off] - ref[off]) / ref[off]
  limit = _dist_bound(np.float64)
  print('isomap golden %s: max |dist_matrix_ - reference| / reference = %.3g = %.3g of the bound %.3g'
        % (backend, rel.max(), rel.max() / limit, limit))
  assert rel.max() <= limit


def test_matches_the_reference_run_cpu():
  _check_golden('numpy')


# ---- the same on the device ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('workers', (1, 4))
def test_matches_scikit_learn_gpu(workers, dtype):
  _check('hip', workers, dtype)


@pytest.mark.gpu
def test_a_disconnected_graph_leaves_zeros_gpu():
  _check_disconnected('hip', np.float32)


@pytest.mark.gpu
def test_refusals_gpu():
  x = np.array(s_curve(np.float32))
  with pytest.raises(NotImplementedError, match='dense'):
    _fit('hip', 1, x, n_neighbors=K, eigen_solver='arpack')
  with pytest.raises(ValueError, match='127'):
    _fit('hip', 1, x, n_neighbors=128)


@pytest.mark.gpu
def test_matches_the_reference_run_gpu():
  _check_golden('hip')
