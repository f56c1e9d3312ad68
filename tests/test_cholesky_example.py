"""The drivers over the dense factorisation kernels: examples/cholesky.py (blocked Cholesky over map2's region join)
and examples/ssvd/qr.py (thin Cholesky-QR).  CPU leg: the host framework on the NumPy oracle backend, where the tile
bodies are LAPACK's, as in the reference.  GPU leg: the same drivers on the HIP backend (sp_potrf, sp_trsm_rlt, the
MFMA GEMM).  Yardsticks: tests/linalg_cases.py; for Q additionally the loss of orthogonality of Cholesky-QR,
||Q^T Q - I||_F <= 8 K u kappa_2(Y)^2 (Yamamoto, Nakatsukasa, Yanagisawa, Fukaya, ETNA 44 (2015), section 3: O(u kappa^2)
without constants; the factor 8 is a margin).

Grids: 4 workers at N = 128, 130 (cells of 65) and 2 * 256 + 2 (cells one past the kernel's outer block); 9 workers at
N = 192 (uneven row tiles under the 3 x 3 grid of cells) and at N = 198 = 9 * 22 (nine equal row tiles)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples.cholesky import cholesky
from spartan_amd.examples.ssvd.qr import qr
from tests import linalg_cases as lc

DTYPES = (np.float32, np.float64)
GRIDS = ((4, 128), (4, 130), (4, 2 * lc.OB + 2), (9, 192), (9, 198))
TALL = ((4096, 64), (1000, 33))


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _check_cholesky(backend, workers, n, dtype):
  a = lc.spd(n, dtype)
  _start(backend, workers)
  try:
    low = cholesky(sp.from_numpy(a)).glom()
  finally:
    sp.shutdown()
  assert low.dtype == np.dtype(dtype) and low.shape == a.shape
  assert not np.any(np.triu(low, 1))
  ratio = lc.potrf_ratio(a, low)
  print('cholesky %s w=%d N=%d %s: ||A - L L^T|| / bound = %.4g' % (backend, workers, n, np.dtype(dtype).name, ratio))
  assert ratio <= 1.0
  return low


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('workers,n', GRIDS)
def test_cholesky_cpu(workers, n, dtype):
  low = _check_cholesky('numpy', workers, n, dtype)
  if np.dtype(dtype) == np.float64:
    # rtol = 1e-12 on the scale of the factor.  Entry by entry alone it cannot hold for ANY second implementation: an
    # entry that is small by cancellation (1e-5 here, beside entries of 10 to 30) carries the absolute rounding error
    # of its row, a few u |L|_max, and the blocked order of the driver and LAPACK's recursive order differ there by
    # 3e-17 to 3e-16 absolute (measured: 1 to 11 entries per case, relative 1.6e-12 to 4.2e-11 of their own size).
    want = np.linalg.cholesky(lc.spd(n, dtype))
    np.testing.assert_allclose(low, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('workers,n', GRIDS)
def test_cholesky_gpu(workers, n, dtype):
  _check_cholesky('hip', workers, n, dtype)


def test_cholesky_cpu_matches_the_reference_run():
  """tests/golden/cholesky_w4.npz: the reference's own driver at 4 workers on the N = 128 input
  (tests/golden/make_golden_linalg.py), entry by entry (the two runs make the same LAPACK calls on the same cells)."""
  import os
  gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cholesky_w4.npz'))
  assert gold['a'].tobytes() == lc.spd(128, np.float64).tobytes()
  low = _check_cholesky('numpy', 4, 128, np.float64)
  diff = np.abs(low - gold['l'])
  print('max |L - L_reference| = %.3g, elementwise relative %.3g' % (diff.max(), (diff / np.abs(gold['l']).clip(1e-300)).max()))
  np.testing.assert_allclose(low, gold['l'], rtol=1e-12)


def test_cholesky_refusals_cpu():
  _start('numpy', 4)
  try:
    with pytest.raises(ValueError):
      cholesky(sp.from_numpy(np.ones((8, 6))))
    with pytest.raises(ValueError):
      cholesky(sp.from_numpy(np.eye(7)))
    bad = lc.spd(128, np.float64).copy()
    bad[70, 70] = -1
    with pytest.raises(np.linalg.LinAlgError):
      cholesky(sp.from_numpy(bad)).glom()
  finally:
    sp.shutdown()


def _tall(shape, dtype):
  return np.random.RandomState(20150708).randn(*shape).astype(dtype)


def _check_qr(backend, workers, shape, dtype):
  y = _tall(shape, dtype)
  k = shape[1]
  _start(backend, workers)
  try:
    q_arr, r = qr(sp.from_numpy(y))
    q = q_arr.glom()
  finally:
    sp.shutdown()
  assert isinstance(r, np.ndarray) and r.dtype == np.dtype(dtype) and r.shape == (k, k)
  assert q.dtype == np.dtype(dtype) and q.shape == shape
  assert not np.any(np.tril(r, -1)) and np.all(np.diag(r) > 0)
  q64, r64, y64 = q.astype(np.float64), r.astype(np.float64), y.astype(np.float64)
  resid = lc.fro(q64.dot(r64) - y64) / (lc.gamma(k + 1, dtype) * lc.fro(np.abs(q64).dot(np.abs(r64))))
  sv = np.linalg.svd(y64, compute_uv=False)
  ortho = lc.fro(q64.T.dot(q64) - np.eye(k)) / (8 * k * lc.U[np.dtype(dtype)] * (sv[0] / sv[-1]) ** 2)
  print('qr %s w=%d %s %s: ||QR - Y|| / bound = %.4g, ||Q^T Q - I|| / bound = %.4g'
        % (backend, workers, shape, np.dtype(dtype).name, resid, ortho))
  assert resid <= 1.0
  assert ortho <= 1.0


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', TALL, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('workers', (1, 4))
def test_qr_cpu(workers, shape, dtype):
  _check_qr('numpy', workers, shape, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', TALL, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('workers', (1, 4))
def test_qr_gpu(workers, shape, dtype):
  _check_qr('hip', workers, shape, dtype)
