"""examples/spectral_clustering and examples/lanczos on the injected NumPy backend, where the tile bodies are the NumPy
restatements beside the driver (examples/_spectral.py).  The same checks on the HIP backend are in
tests/test_spectral_gpu.py.

Input: tests/spectral_cases.planted -- 60 points in 2-D in three planted groups, k = 3, num_iter = 5.  Yardstick:
tests/golden/spectral_w4.npz, recorded by tests/golden/make_golden_spectral.py from the reference's own mappers, its
lanczos.solve at rank 6 and its whole spectral_cluster at 4 workers.

Labels are compared as partitions (sets of sets): label numbers are free.  Ritz values: |d - golden| <= 2 e_L, e_L the
largest entry of the derived bound of L (tests/spectral_cases.eps): by Weyl's inequality the eigenvalues of L + E move
by at most ||E||_2 <= e_L ||L||_2, and ||L||_2 <= 2 because the normalised part has spectral radius 1 and the
overwritten diagonal adds less than 1.  Weyl bounds eigenvalues, not eight-step Ritz values; that these respond alike
on this input was found by experiment (20 random symmetric relative perturbations of L at each of 1e-15, 1e-12, 1e-7 and
1e-5 moved the three leading Ritz values by about 0.2 times the perturbation).  The share of the limit is printed."""
import functools
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples import lanczos
from spartan_amd.examples.spectral_clustering import affinity_matrix, laplacian, spectral_cluster
from tests import spectral_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
K, NUM_ITER, RANK = 3, 5, 6


@functools.lru_cache(maxsize=None)
def golden():
  g = dict(np.load(os.path.join(HERE, 'golden', 'spectral_w4.npz')))
  assert g['points'].tobytes() == sc.planted()[0].tobytes()
  return g


@functools.lru_cache(maxsize=None)
def ritz_limit(dtype):
  """2 e_L for a run in `dtype` on the planted input."""
  p = sc.planted()[0].astype(dtype)
  return 2 * float(sc.eps(sc.oracle(p, 'rbf'), p.shape[1], 'rbf', dtype)['L'].max())


def start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def tiled(x, workers):
  return sp.from_numpy(x, tile_hint=(-(-x.shape[0] // workers), x.shape[1])) if workers > 1 else sp.from_numpy(x)


def check_driver(backend, workers, dtype, extra=0.0):
  """The whole driver on the planted input: both partitions, and the Ritz values within 2 e_L + extra of the golden's."""
  g = golden()
  p, truth = sc.planted()
  start(backend, workers)
  try:
    labels, d, u, deg = spectral_cluster(tiled(p.astype(dtype), workers), K, NUM_ITER, full_output=True)
    assert tuple(labels.shape)[0] == 60
    got = np.asarray(labels.glom()).reshape(-1)
    assert d.shape == (RANK,) and u.shape == (60, K) and deg.shape == (60,) and deg.dtype == np.dtype(dtype)
    limit = ritz_limit(np.dtype(dtype)) + extra
    err = float(np.abs(d - g['lanczos_d']).max())
    print('spectral_cluster %s %d workers %s: max |Ritz values - golden| = %.3g, %.3g of the limit %.3g'
          % (backend, workers, np.dtype(dtype).name, err, err / limit, limit))
    assert sc.partition(got) == sc.partition(truth)
    assert sc.partition(got) == sc.partition(g['labels_w4']) == sc.partition(g['labels'])
    assert err <= limit
  finally:
    sp.shutdown()


def check_laplacian_bits(backend, dtype):
  """L and D at 1, 3 and 4 workers: the same bits, symmetric bit for bit, a diagonal of 1, inside the bound."""
  p = sc.planted()[0].astype(dtype)
  want = sc.oracle(p, 'rbf')
  seen = []
  for workers in (1, 3, 4):
    start(backend, workers)
    try:
      lap, deg = laplacian(tiled(p, workers))
      lap = np.asarray(lap.glom())
      a = np.asarray(affinity_matrix(tiled(p, workers), 'manhattan').glom())
    finally:
      sp.shutdown()
    sc.check(p, 0, 60, 'rbf', want, deg=deg, lap=lap, label='laplacian %s %d workers %s' % (backend, workers, np.dtype(dtype).name))
    assert lap.tobytes() == lap.T.tobytes() and a.tobytes() == a.T.tobytes()
    seen.append(lap.tobytes() + deg.tobytes() + a.tobytes())
  assert seen[0] == seen[1] == seen[2]


def check_refusals(backend):
  p = sc.planted()[0]
  start(backend, 1)
  try:
    x = sp.from_numpy(p)
    with pytest.raises(NotImplementedError, match='np.square'):
      spectral_cluster(x, K, NUM_ITER, 'scaled_euclidean')
    with pytest.raises(ValueError, match='unknown metric'):
      spectral_cluster(x, K, NUM_ITER, 'cosine')
    with pytest.raises(ValueError, match='gamma'):
      spectral_cluster(x, K, NUM_ITER, gamma=float('nan'))
    with pytest.raises(ValueError, match='k = 0'):
      spectral_cluster(x, 0)
    with pytest.raises(ValueError, match='k = 61'):
      spectral_cluster(x, 61)
    with pytest.raises(ValueError, match='num_iter'):
      spectral_cluster(x, K, 0)
    with pytest.raises(ValueError, match='shape'):
      spectral_cluster(sp.from_numpy(p.reshape(-1)), K)
    with pytest.raises(TypeError, match='float32 float64'):
      spectral_cluster(x, K, dtype=np.int32)
    # integer points are converted to float64; the other two measures run
    ints = np.round(p * 4).astype(np.int32)
    got = np.asarray(spectral_cluster(sp.from_numpy(ints), K, NUM_ITER).glom()).reshape(-1)
    want = np.asarray(spectral_cluster(sp.from_numpy(ints.astype(np.float64)), K, NUM_ITER).glom()).reshape(-1)
    assert sc.partition(got) == sc.partition(want)
    for metric in ('euclidean', 'manhattan'):
      labels = np.asarray(spectral_cluster(x, K, 2, metric).glom()).reshape(-1)
      assert labels.shape == (60,) and labels.min() >= 0 and labels.max() < K
  finally:
    sp.shutdown()


@pytest.mark.parametrize('workers', (1, 4))
def test_lanczos_reproduces_the_reference_ritz_values(workers):
  g = golden()
  start('numpy', workers)
  try:
    lap = sp.from_numpy(g['L_rbf'], tile_hint=(60 // workers, 60)).evaluate()
    d, s = lanczos.solve(lap, lap, RANK, True)
    d2, _ = lanczos.solve(lap, lap, RANK, False)          # dot(AT, dot(A, v)): the squares
  finally:
    sp.shutdown()
  limit = ritz_limit(np.dtype(np.float64))
  err = float(np.abs(d - g['lanczos_d']).max())
  print('lanczos.solve numpy %d workers: max |d - golden| = %.3g, %.3g of the limit %.3g' % (workers, err, err / limit, limit))
  assert d.shape == (RANK,) and s.shape == (60, RANK) and err <= limit
  # the Ritz vectors up to the sign numpy.linalg.eig gives them
  dots = np.abs(np.sum(s[:, :3] * g['lanczos_s'][:, :3], axis=0))
  assert np.all(np.abs(dots - 1) < 1e-8), dots
  # (eight steps on L^2 are another Krylov space: its Ritz values are near the squares, not at them)
  assert np.all(np.abs(np.sqrt(d2[:3]) - g['lanczos_d'][:3]) < 1e-3)


def test_lanczos_breakdown_is_an_error():
  start('numpy', 1)
  try:
    eye = sp.from_numpy(np.eye(6)).evaluate()             # ones / sqrt(n) is an eigenvector: beta_1 = 0
    with pytest.raises(np.linalg.LinAlgError, match='breakdown'):
      lanczos.solve(eye, eye, 2, True)
  finally:
    sp.shutdown()


@pytest.mark.parametrize('workers', (1, 3, 4))
def test_the_sign_of_the_ritz_vectors_and_the_kmeans_reducer(workers):
  """Why the driver fits KMeans with reducer=np.add.  numpy.linalg.eig gives the Ritz vectors either sign (the golden
  run drew +; a change of 1e-16 in L draws the other), and the sign decides the starting rows U[argmax(U, axis=0)]: with
  -U two of them lie in the same group.  The real update recovers from either start at any number of workers; the
  reference's default -- the last tile's partial sums replace the others' -- recovers from -U only with one tile."""
  from spartan_amd.examples.sklearn.cluster.k_means_ import KMeans
  g = golden()
  outcome = {}
  start('numpy', workers)
  try:
    for sign in (1, -1):
      u = np.ascontiguousarray(sign * g['lanczos_s'][:, :K])
      init = u[np.argmax(u, axis=0)]
      if sign < 0:
        assert len(set((np.argmax(u, axis=0) % 3).tolist())) == 2          # two starting rows in one planted group
      for reducer in (None, np.add):
        _, labels = KMeans(K, NUM_ITER).fit(sp.from_numpy(u), init, reducer=reducer)
        found = sc.partition(np.asarray(labels.glom()).reshape(-1)) == sc.partition(g['truth'])
        outcome[sign, reducer is not None] = found
  finally:
    sp.shutdown()
  print('KMeans on +-U at %d workers, (sign, reducer=np.add) -> planted groups found: %s' % (workers, outcome))
  assert outcome[1, True] and outcome[-1, True]            # the driver's choice: either sign, any number of workers
  assert outcome[1, False]                                 # the golden run's sign: the reference's default finds them too
  assert outcome[-1, False] == (workers == 1)              # the other sign: only where there is a single tile


@pytest.mark.parametrize('workers', (1, 4))
def test_the_driver_finds_the_planted_groups_cpu(workers):
  check_driver('numpy', workers, np.float64)


def test_the_laplacian_does_not_depend_on_the_workers_cpu():
  check_laplacian_bits('numpy', np.float64)


def test_refusals_cpu():
  check_refusals('numpy')
