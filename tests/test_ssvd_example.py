"""The drivers over the symmetric eigensolver: examples/ssvd/ssvd.py (stochastic SVD) and examples/pca.py.  CPU leg: the
host framework on the NumPy oracle backend at 1 and 4 workers, where the dense tile bodies are LAPACK's.  GPU leg: the
same drivers on the HIP backend (the MFMA GEMM, sp_potrf, sp_trsm_rlt, sp_syevj).

svd: A = X . diag(s) . Y^T of exact rank k (1000 x 40; k = 8 and 33; s spread over [1, 2]) with Omega passed in.  Since
range(A . Omega) = range(A), the answer is the exact thin SVD of A whatever Omega is; it is measured against the
float64 LAPACK SVD of the stored A.  Yardstick: the reference's own recipe (inv(R), numpy.linalg.eigh, the same
Omega) transcribed in NumPy in the dtype under test; each error may be 8 times the transcription's or k u, whichever
is larger (the Gram steps square kappa(Y), and the two routes round it differently).

PCA: 600 x 12 float64 data, a planted 3-dimensional subspace plus noise 1e-3 (float64 only: at rank 12 the centred
data has kappa ~ 1e4 and Cholesky-QR needs kappa^2 u < 1, in the reference's recipe as here)."""
import functools

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.array import distarray
from spartan_amd.examples.pca import PCA
from spartan_amd.examples.ssvd.ssvd import svd
from tests import eig_cases as ec

DTYPES = (np.float32, np.float64)
M, N = 1000, 40
RANKS = (8, 33)
MARGIN = 8.0


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


@functools.lru_cache(maxsize=None)
def _problem(k, dtype):
  rng = np.random.RandomState(20150708)
  x = np.linalg.qr(rng.randn(M, k))[0]
  y = np.linalg.qr(rng.randn(N, k))[0]
  a = (x * np.linspace(2.0, 1.0, k)).dot(y.T).astype(dtype)
  omega = rng.randn(N, k).astype(dtype)
  u64, s64, vt64 = np.linalg.svd(a.astype(np.float64), full_matrices=False)
  for v in (a, omega):
    v.setflags(write=False)
  return a, omega, s64[:k]


def _errors(a, k, u, s, vt):
  a64, u64, s64, vt64 = (np.asarray(v, np.float64) for v in (a, u, s, vt))
  want = np.linalg.svd(a64, compute_uv=False)[:k]
  return (float(np.abs(s64 - want).max() / want.max()),
          ec.fro((u64 * s64).dot(vt64) - a64) / ec.fro(a64),
          ec.fro(u64.T.dot(u64) - np.eye(k)))


@functools.lru_cache(maxsize=None)
def _recipe_errors(k, dtype):
  """The reference's ssvd.py and qr.py line by line in NumPy, in the dtype under test, with eigh for eig."""
  a, omega, _ = _problem(k, dtype)
  y = a.dot(omega)
  r = np.linalg.cholesky(y.T.dot(y)).T
  q = y.dot(np.linalg.inv(r))
  b = q.T.dot(a)
  w, vecs = np.linalg.eigh(b.dot(b.T))
  s = np.sqrt(np.maximum(w, 0))[::-1]
  vecs = vecs[:, ::-1]
  u = q.dot(vecs)
  vt = (b.T.dot(vecs) * (np.ones(k, s.dtype) / s)).T
  assert u.dtype == a.dtype
  return _errors(a, k, u, s, vt)


def _check_svd(backend, workers, k, dtype):
  a, omega, _ = _problem(k, dtype)
  _start(backend, workers)
  try:
    arr = sp.from_numpy(a)
    row_tiles = sorted((ex.ul[0], ex.lr[0]) for ex in arr.evaluate().tiles)
    U, s, vt = svd(arr, k, omega=omega)
    assert isinstance(U, distarray.DistArray) and tuple(U.shape) == (M, k)
    assert sorted((ex.ul[0], ex.lr[0]) for ex in U.tiles) == row_tiles and all(ex.shape[1] == k for ex in U.tiles)
    u = U.glom()
  finally:
    sp.shutdown()
  assert isinstance(s, np.ndarray) and s.shape == (k,) and s.dtype == np.dtype(dtype)
  assert isinstance(vt, np.ndarray) and vt.shape == (k, N) and vt.dtype == np.dtype(dtype)
  assert u.dtype == np.dtype(dtype)
  assert np.all(s[:-1] >= s[1:])
  got, yard = _errors(a, k, u, s, vt), _recipe_errors(k, np.dtype(dtype))
  floor = k * ec.U[np.dtype(dtype)]
  ok = True
  for name, g, y in zip(('S', 'U S V - A', 'U^T U - I'), got, yard):
    limit = max(MARGIN * y, floor)
    print('svd %s w=%d k=%d %s: error of %s = %.4g  limit %.4g (recipe %.4g, k u %.4g)'
          % (backend, workers, k, np.dtype(dtype).name, name, g, limit, y, floor))
    ok = ok and g <= limit
  assert ok, (got, yard)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('k', RANKS)
@pytest.mark.parametrize('workers', (1, 4))
def test_svd_cpu(workers, k, dtype):
  _check_svd('numpy', workers, k, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('k', RANKS)
@pytest.mark.parametrize('workers', (1, 4))
def test_svd_gpu(workers, k, dtype):
  _check_svd('hip', workers, k, dtype)


def test_svd_draws_its_own_omega_and_refuses_a_wrong_one_cpu():
  a, omega, _ = _problem(8, np.float64)
  _start('numpy', 4)
  try:
    U, s, vt = svd(sp.from_numpy(a), 8)
    assert ec.fro((U.glom() * s).dot(vt) - a) / ec.fro(a) < 1e-10
    U, s, vt = svd(sp.from_numpy(a[:, :6]))                       # k defaults to the number of columns
    assert tuple(U.shape) == (M, 6) and s.shape == (6,) and vt.shape == (6, 6)
    with pytest.raises(ValueError):
      svd(sp.from_numpy(a), 8, omega=omega[:, :5])
  finally:
    sp.shutdown()


# ---- PCA
@functools.lru_cache(maxsize=None)
def _pca_data():
  rng = np.random.RandomState(20150708)
  basis = np.linalg.qr(rng.randn(12, 3))[0]
  x = (rng.randn(600, 3) * (3.0, 2.0, 1.0)).dot(basis.T) + rng.randn(12) + 1e-3 * rng.randn(600, 12)
  omega = rng.randn(12, 12)
  for v in (x, omega):
    v.setflags(write=False)
  return x, omega


def _angles(components, centred):
  """The sines of the principal angles between the row space of `components` (3 x 12) and the leading three right
  singular vectors of the centred data."""
  want = np.linalg.svd(centred, full_matrices=False)[2][:3]
  q = np.linalg.qr(np.asarray(components, np.float64).T)[0]
  cos = np.linalg.svd(want.dot(q), compute_uv=False)
  return np.sqrt(np.maximum(0.0, 1.0 - np.minimum(cos, 1.0) ** 2))


@functools.lru_cache(maxsize=None)
def _pca_recipe_angle():
  x, omega = _pca_data()
  c = x - x.mean(axis=0)
  y = c.dot(omega)
  r = np.linalg.cholesky(y.T.dot(y)).T
  q = y.dot(np.linalg.inv(r))
  b = q.T.dot(c)
  w, vecs = np.linalg.eigh(b.dot(b.T))
  s = np.sqrt(np.maximum(w, 0))[::-1]
  vt = (b.T.dot(vecs[:, ::-1]) * (1.0 / s)).T
  return float(_angles(vt[:3], c).max())


def _check_pca(backend, workers):
  x, omega = _pca_data()
  _start(backend, workers)
  try:
    arr = sp.from_numpy(x.copy())
    pca = PCA(n_components=3)
    assert pca.fit(arr, rank=12, omega=omega) is pca
    assert np.array_equal(arr.glom(), x)                           # the caller's X is unchanged
    assert isinstance(pca.components_, np.ndarray) and pca.components_.shape == (3, 12)
    low = pca.transform(arr)
    assert isinstance(low, np.ndarray) and low.shape == (600, 3)
    back_host = pca.inverse_transform(low)
    back_dist = pca.inverse_transform(sp.from_numpy(low))
    assert isinstance(back_host, np.ndarray) and isinstance(back_dist, distarray.DistArray)
    back_dist = back_dist.glom()
    mean = pca.mean_.glom()
  finally:
    sp.shutdown()
  np.testing.assert_allclose(mean, x.mean(axis=0), rtol=1e-12)
  angle, yard = float(_angles(pca.components_, x - x.mean(axis=0)).max()), _pca_recipe_angle()
  limit = max(MARGIN * yard, 12 * ec.U[np.dtype(np.float64)])
  print('pca %s w=%d: largest principal angle (sine) = %.4g  limit %.4g (recipe %.4g)' % (backend, workers, angle, limit, yard))
  assert angle <= limit
  # nine directions of noise 1e-3 are dropped: 600 x 12 entries of it, less the three kept, stay in the residual
  for back in (back_host, back_dist):
    assert back.shape == x.shape
    err = ec.fro(back - x) / np.sqrt(x.size)
    print('pca %s w=%d: rms of inverse_transform(transform(X)) - X = %.4g (noise 1e-3)' % (backend, workers, err))
    assert err <= 1e-3 and np.abs(back - x).max() <= 6e-3
  np.testing.assert_allclose(back_dist, back_host, rtol=0, atol=1e-12 * np.abs(x).max())


@pytest.mark.parametrize('workers', (1, 4))
def test_pca_cpu(workers):
  _check_pca('numpy', workers)


@pytest.mark.gpu
@pytest.mark.parametrize('workers', (1, 4))
def test_pca_gpu(workers):
  _check_pca('hip', workers)
