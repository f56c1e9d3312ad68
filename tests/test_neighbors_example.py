"""examples/sklearn/neighbors: the NearestNeighbors driver.  CPU leg: the host framework on the injected NumPy backend,
where the tile bodies are the NumPy helpers beside the driver (examples/sklearn/neighbors/_knn.py).  GPU leg: the same
driver on the HIP backend (sp_knn, sp_knn_merge, the map kernel's sqrt).  Oracle and bounds: tests/knn_cases.py, applied
to dist**2 (squared in float64: the square root the driver takes and this square add two roundings of the result's
dtype, far inside gamma = (d + 2) u at d = 33); tests/golden/knn_w4.npz: the reference's own driver at 4 workers."""
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples.sklearn.neighbors import NearestNeighbors
from tests import knn_cases as kc

HERE = os.path.dirname(os.path.abspath(__file__))
NQ, NP, D, K = 37, 1031, 33, 17


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _run(backend, workers, q, x, k, algorithm, tile_hint=None, as_numpy=False, k_at_call=None):
  ctx = _start(backend, workers)
  try:
    fitted = x if as_numpy else sp.from_numpy(x, tile_hint=tile_hint)
    nn = NearestNeighbors(n_neighbors=k, algorithm=algorithm).fit(fitted)
    dist, ind = nn.kneighbors(q if as_numpy else sp.from_numpy(q), n_neighbors=k_at_call)
    launches = getattr(ctx.backend, 'launches', None)
  finally:
    sp.shutdown()
  k = k_at_call or k
  assert isinstance(dist, np.ndarray) and isinstance(ind, np.ndarray)
  assert dist.shape == (q.shape[0], k) and ind.shape == (q.shape[0], k) and ind.dtype == np.int64
  return dist, ind, launches


def _check_real(backend, workers, algorithm, dtype, tile_hint=None, **kw):
  q, x = kc.real_case(NQ, NP, D, dtype)
  dist, ind, _ = _run(backend, workers, q, x, K, algorithm, tile_hint, **kw)
  assert dist.dtype == np.dtype(dtype)
  kc.check_real(dist.astype(np.float64) ** 2, ind, q, x, K, d2_dtype=dtype,
                label='%s w=%d %s' % (backend, workers, algorithm))


def _check_integer(backend, workers, algorithm, dtype, tile_hint=None):
  q, x = kc.integer_case(NQ, NP, D, dtype)
  dist, ind, _ = _run(backend, workers, q, x, K, algorithm, tile_hint)
  want_d, want_i = kc.oracle(q, x, K)
  np.testing.assert_array_equal(ind, want_i)
  assert dist.tobytes() == np.sqrt(want_d.astype(dtype)).tobytes()       # dist == sqrt(d2), elementwise


@pytest.mark.parametrize('algorithm', ('auto', 'kd_tree', 'brute'))
@pytest.mark.parametrize('workers', (1, 3, 4, 8))
def test_real_inputs_cpu(workers, algorithm):
  _check_real('numpy', workers, algorithm, np.float64)


@pytest.mark.parametrize('algorithm', ('auto', 'ball_tree', 'brute'))
def test_real_inputs_float32_cpu(algorithm):
  _check_real('numpy', 4, algorithm, np.float32)


@pytest.mark.parametrize('algorithm', ('auto', 'brute'))
def test_x_cut_by_columns_as_well_cpu(algorithm):
  _check_real('numpy', 4, algorithm, np.float64, tile_hint=(300, 17))


@pytest.mark.parametrize('algorithm', ('auto', 'kd_tree', 'brute'))
@pytest.mark.parametrize('workers', (1, 3, 4, 8))
def test_integer_inputs_exactly_cpu(workers, algorithm):
  _check_integer('numpy', workers, algorithm, np.float64)


def test_interface_cpu():
  q, x = kc.integer_case(9, 40, 3, np.float64)
  want_d, want_i = kc.oracle(q, x, 3)
  for algorithm in ('auto', 'brute'):
    dist, ind, _ = _run('numpy', 3, q, x, 5, algorithm, k_at_call=3)           # n_neighbors of the call wins
    np.testing.assert_array_equal(ind, want_i)
    dist, ind, _ = _run('numpy', 3, q, x, 3, algorithm, as_numpy=True)        # NumPy inputs
    np.testing.assert_array_equal(ind, want_i)
    assert dist.tobytes() == np.sqrt(want_d.astype(np.float64)).tobytes()
    with pytest.raises(ValueError, match='n_neighbors'):
      _run('numpy', 3, q, x, 41, algorithm)
  with pytest.raises(ValueError):
    _run('numpy', 3, q, x, 3, 'quantum')
  with pytest.raises(ValueError):
    _run('numpy', 3, q[:, :2], x, 3, 'auto')
  assert NearestNeighbors().n_neighbors == 5 and NearestNeighbors().algorithm == 'auto'


def _golden():
  gold = np.load(os.path.join(HERE, 'golden', 'knn_w4.npz'))
  q, x = kc.real_case(NQ, NP, D, np.float64)
  assert gold['q'].tobytes() == q.tobytes() and gold['x'].tobytes() == x.tobytes()
  return gold, q, x


def _check_golden(backend):
  """The reference's own NearestNeighbors(5, 'kd_tree') at 4 workers (tests/golden/make_golden_knn.py): the same
  indices -- the recorded distances of a row are more than 4 gamma apart -- and distances within gamma (relative)."""
  gold, q, x = _golden()
  g = kc.gamma(D, np.float64)
  for algorithm in ('kd_tree', 'brute'):
    dist, ind, _ = _run(backend, 4, q, x, 5, algorithm)
    # (the reference's own 'brute' run is in the file too: its indices, floats there, are those of its kd_tree run)
    ref = gold['dist'] if algorithm == 'kd_tree' else gold['brute_dist']
    np.testing.assert_array_equal(ind, gold['ind'])
    np.testing.assert_array_equal(ind, gold['brute_ind'].astype(np.int64))
    rel = np.abs(dist - ref) / ref
    print('knn golden %s %s: max |dist - reference| / reference = %.3g (gamma = %.3g)' % (backend, algorithm, rel.max(), g))
    assert np.all(np.abs(dist - ref) <= g * ref)


def test_matches_the_reference_run_cpu():
  _check_golden('numpy')


def test_two_ranks_cpu():
  """One process per rank: 4 workers over 2 ranks (tests/mp_knn_worker.py); every rank checks the merged result."""
  from tests.test_multiprocess import _run_ranks
  _run_ranks(2, 'mp_knn_worker.py', ['4'])


# ---- the same on the device ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('workers', (1, 4))
def test_real_and_integer_inputs_gpu(workers, dtype):
  _check_real('hip', workers, 'auto', dtype)
  _check_integer('hip', workers, 'auto', dtype)


@pytest.mark.gpu
def test_x_cut_by_columns_as_well_gpu():
  _check_real('hip', 4, 'auto', np.float32, tile_hint=(300, 17))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_auto_and_brute_agree_with_the_oracle_gpu(dtype):
  q, x = kc.integer_case(9, 40, 3, dtype)
  want_d, want_i = kc.oracle(q, x, 5)
  for algorithm in ('auto', 'brute'):
    dist, ind, _ = _run('hip', 3, q, x, 5, algorithm)
    np.testing.assert_array_equal(ind, want_i)
    assert dist.tobytes() == np.sqrt(want_d.astype(dtype)).tobytes()


@pytest.mark.gpu
def test_launches_do_not_grow_with_the_number_of_points_gpu():
  """Four row bands of X at np = 1031 and at np = 4124: the same number of launches, so nothing per row runs on the
  host."""
  counts = []
  for npts in (NP, 4 * NP):
    q, x = kc.integer_case(NQ, npts, D, np.float32)
    _, _, launches = _run('hip', 4, q, x, K, 'auto', tile_hint=((npts + 3) // 4, D))
    counts.append(launches)
  print('launches of one kneighbors at 4 tiles: np=%d: %d, np=%d: %d' % (NP, counts[0], 4 * NP, counts[1]))
  assert counts[0] == counts[1] and counts[0] > 0


@pytest.mark.gpu
def test_matches_the_reference_run_gpu():
  _check_golden('hip')


@pytest.mark.gpu
def test_two_ranks_hip_shared_gpu():
  from tests.test_multiprocess import _run_ranks
  _run_ranks(2, 'mp_knn_worker.py', ['4', 'hip'])
