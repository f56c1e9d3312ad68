"""examples/fuzzy_kmeans: the fuzzy k-means driver.  CPU leg: the host framework on the injected NumPy backend, where
the tile body is the NumPy restatement beside the driver (examples/_fuzzy.py).  GPU leg: the same checks on the HIP
backend (sp_fuzzy_step).

Input: 96 x 7 points uniform in [0, 1), k = 5 fixed starting centres, m = 2 and 1.5, two iterations.  Yardstick:
tests/golden/fuzzy_w4.npz, the outputs of the reference's own two mappers (cdist, float64) chained over two iterations,
recorded by tests/golden/make_golden_fuzzy.py, which asserts that the two largest memberships of every row differ by at
least 1e-3 relative -- far above the step's bound in float32 (about 1e-5) -- so a float32 run must find the same labels.

Labels are compared exactly.  Centres on the NumPy backend in float64: 1e-10 relative.  Centres on the device: within
b2(T) + b2(float64) per entry, b2 the two-iteration bound of tests/fuzzy_cases.two_step_bound for the dtype under test
(our error) and for float64 (the reference's own, which computes in float64 with the same number of roundings or fewer);
measured against bound is printed.  'fused' must not allocate an n x k tile: on the device the backend's fuzzy_step is
watched and never asked for U."""
import functools
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples.fuzzy_kmeans import fuzzy_kmeans
from tests import fuzzy_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
N, D, K, SEED = 96, 7, 5, 20151068
MS = (2.0, 1.5)
IMPLEMENTATIONS = ('fused', 'map2')


@functools.lru_cache(maxsize=None)
def points():
  x = np.random.RandomState(SEED).rand(N, D)
  x.setflags(write=False)
  return x


@functools.lru_cache(maxsize=None)
def start_centers():
  c = np.random.RandomState(SEED + 1).rand(K, D)
  c.setflags(write=False)
  return c


@functools.lru_cache(maxsize=None)
def golden():
  g = dict(np.load(os.path.join(HERE, 'golden', 'fuzzy_w4.npz')))
  assert g['points'].tobytes() == points().tobytes() and g['centers0'].tobytes() == start_centers().tobytes()
  return g


@functools.lru_cache(maxsize=None)
def center_bound(m, dtype):
  """Per entry, what |ours - golden| may be after two iterations in `dtype` (see the module docstring)."""
  _, _, c2, b2 = fc.two_step_bound(points(), start_centers(), m, dtype)
  _, _, _, b2_ref = fc.two_step_bound(points(), start_centers(), m, np.float64)
  return np.asarray(c2, np.float64), np.asarray(b2 + b2_ref, np.float64)


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _check_driver(backend, workers, dtype, implementation, m):
  g = golden()
  tag = 'm%g_' % m
  ctx = _start(backend, workers)
  try:
    x = points().astype(dtype)
    X = sp.from_numpy(x, tile_hint=(N // workers, D)) if workers > 1 else sp.from_numpy(x)
    asked = []
    step = getattr(ctx.backend, 'fuzzy_step', None)
    if step is not None:                       # watch what the driver asks of the kernel
      def watched(p, c, mm, want_u=False, splits=0):
        asked.append((tuple(p.shape), bool(want_u)))
        return step(p, c, mm, want_u=want_u, splits=splits)
      ctx.backend.fuzzy_step = watched
    try:
      labels, centers = fuzzy_kmeans(X, k=K, num_iter=2, m=m, centers=np.array(start_centers()),
                                     implementation=implementation, full_output=True)
      assert tuple(labels.shape) == (N,)
      got_labels = np.asarray(labels.glom())
    finally:
      if step is not None:
        del ctx.backend.fuzzy_step
    assert got_labels.dtype == np.int64 and centers.dtype == np.dtype(dtype) and centers.shape == (K, D)
    assert got_labels.tobytes() == g[tag + 'labels2'].tobytes()
    if tag + 'labels_w4' in g:
      assert got_labels.tobytes() == g[tag + 'labels_w4'].tobytes()
    want = g[tag + 'centers2']
    err = np.abs(centers.astype(np.float64) - want)
    if backend == 'hip':
      _, bound = center_bound(m, np.dtype(dtype))
      print('fuzzy_kmeans %s %s %d workers %s m=%g: max |centres - golden| = %.3g, %.3g of the two-iteration bound '
            '(largest bound %.3g)' % (backend, implementation, workers, np.dtype(dtype).name, m, err.max(),
                                      (err / bound).max(), bound.max()))
      assert np.all(err <= bound)
      rows = sorted(shape[0] for shape, _ in asked)
      if implementation == 'fused':
        assert asked and not any(want_u for _, want_u in asked)         # no [n, k] tile anywhere
        assert rows == sorted([N // workers] * workers * 2)
      else:
        assert asked and all(want_u for _, want_u in asked)
    else:
      rel = float((err / np.abs(want)).max())
      print('fuzzy_kmeans %s %s %d workers m=%g: centres differ from the golden by %.3g relative'
            % (backend, implementation, workers, m, rel))
      assert rel <= 1e-10
  finally:
    sp.shutdown()


def _check_refusals(backend):
  _start(backend, 1)
  try:
    x, c = np.array(points()), np.array(start_centers())
    for bad in (1.0, 0.5, float('nan')):
      with pytest.raises(ValueError, match='m = '):
        fuzzy_kmeans(sp.from_numpy(x), k=K, m=bad, centers=c)
    with pytest.raises(ValueError, match='k = 0'):
      fuzzy_kmeans(sp.from_numpy(x), k=0)
    with pytest.raises(ValueError, match='num_iter'):
      fuzzy_kmeans(sp.from_numpy(x), k=K, num_iter=0, centers=c)
    with pytest.raises(ValueError, match='centers of shape'):
      fuzzy_kmeans(sp.from_numpy(x), k=K + 1, centers=c)
    with pytest.raises(ValueError, match='implementation'):
      fuzzy_kmeans(sp.from_numpy(x), k=K, centers=c, implementation='outer')
    # the default start (the reference's rand) runs; integer points are converted on the way in
    labels = np.asarray(fuzzy_kmeans(sp.from_numpy(x), k=3, num_iter=1).glom())
    assert labels.shape == (N,) and labels.min() >= 0 and labels.max() < 3
    ints = (x * 10).astype(np.int32)
    got = np.asarray(fuzzy_kmeans(sp.from_numpy(ints), k=K, num_iter=1, centers=c * 10).glom())
    want = np.asarray(fuzzy_kmeans(sp.from_numpy(ints.astype(np.float64)), k=K, num_iter=1, centers=c * 10).glom())
    assert got.tobytes() == want.tobytes()
  finally:
    sp.shutdown()


def test_the_golden_holds_the_reference_run():
  g = golden()
  for m in MS:
    tag = 'm%g_' % m
    for it in ('1', '2'):
      fuzzy = g[tag + 'fuzzy' + it]
      assert fuzzy.shape == (N, K) and g[tag + 'centers' + it].shape == (K, D)
      assert np.allclose(fuzzy.sum(axis=1), 1.0, rtol=1e-12, atol=0)
      assert g[tag + 'labels' + it].tobytes() == np.argmax(fuzzy, axis=1).astype(np.int64).tobytes()
      top = np.sort(fuzzy, axis=1)
      assert ((top[:, -1] - top[:, -2]) / top[:, -1]).min() >= 1e-3
    # the reference's label is the FARTHEST centre
    d = np.linalg.norm(points()[:, None, :] - start_centers()[None, :, :], axis=2)
    assert g[tag + 'labels1'].tobytes() == np.argmax(d, axis=1).astype(np.int64).tobytes()
    if tag + 'labels_w4' in g:                 # the reference's whole fuzzy_kmeans() at 4 workers
      assert g[tag + 'labels_w4'].tobytes() == g[tag + 'labels2'].tobytes()


@pytest.mark.parametrize('workers', (1, 3, 4))
@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('implementation', IMPLEMENTATIONS)
def test_the_driver_reproduces_the_reference_cpu(implementation, m, workers):
  _check_driver('numpy', workers, np.float64, implementation, m)


def test_refusals_cpu():
  _check_refusals('numpy')


# ---- the same on the device ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('workers', (1, 4))
@pytest.mark.parametrize('implementation', IMPLEMENTATIONS)
def test_the_driver_reproduces_the_reference_gpu(implementation, workers, dtype):
  for m in MS:
    _check_driver('hip', workers, dtype, implementation, m)


@pytest.mark.gpu
def test_refusals_gpu():
  _check_refusals('hip')
