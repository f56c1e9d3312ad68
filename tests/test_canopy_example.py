"""examples/canopy_clustering: the canopy clustering driver.  CPU leg: the host framework on the injected NumPy backend
at 1 and 4 logical workers, where the tile bodies are the NumPy restatements beside the driver (examples/_canopy.py).
GPU leg (marked): the same checks on the HIP backend (sp_canopy, sp_pdf_label).

Reference: tests/golden/canopy_w4.npz, recorded by tests/golden/make_golden_canopy.py from the reference's own mappers
and find_centers at 4 bands (160 rows, float64, four settings of d, t1, t2).  The recording script asserts that no
distance is within 1e-6 of a threshold and no two leading pdfs within 1e-9, so float64 results are compared byte for
byte."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import expr
from spartan_amd.examples import _canopy, canopy_clustering as cc
from tests import canopy_cases as case

BACKENDS = ('numpy', pytest.param('hip', marks=pytest.mark.gpu))
SETTINGS = range(len(case.SETTINGS))


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


@pytest.mark.parametrize('s', SETTINGS)
@pytest.mark.parametrize('workers', (1, 4))
@pytest.mark.parametrize('backend', BACKENDS)
def test_the_golden_run(backend, workers, s):
  """4 workers x 1 chain, or 1 worker x 4 chains: the reference's four tiles either way."""
  g = case.golden()
  x, t1, t2 = case.golden_input(s)
  _start(backend, workers)
  try:
    asked, body = [], _canopy.canopy

    def watched(xt, a1, a2, chains=1, cap=None):
      asked.append((tuple(xt.shape), chains))
      return body(xt, a1, a2, chains=chains, cap=cap)
    _canopy.canopy = watched
    try:
      labels, centers = cc.canopy_cluster(x, t1, t2, case.CF, chains_per_tile=case.WORKERS // workers, return_centers=True)
    finally:
      _canopy.canopy = body
    # one tile body per band, then find_centers' one chain over the bands' results
    per_band = sum(len(g['band_%d_%d' % (s, b)]) for b in range(case.WORKERS))
    assert asked == [((case.ROWS // workers, x.shape[1]), case.WORKERS // workers)] * workers + [((per_band, x.shape[1]), 1)]
    assert case.same(centers, g['centers_%d' % s])
    assert tuple(labels.shape) == (case.ROWS,)
    got = np.asarray(labels.glom())
    assert case.same(got, g['labels_%d' % s])
    # the default call returns the labels alone
    alone = cc.canopy_cluster(x, t1, t2, case.CF, chains_per_tile=case.WORKERS // workers)
    assert case.same(np.asarray(alone.glom()), got)
  finally:
    sp.shutdown()


@pytest.mark.parametrize('backend', BACKENDS)
def test_find_centers_is_the_reference(backend):
  g = case.golden()
  _start(backend, 1)
  try:
    for s in SETTINGS:
      _, t1, t2 = case.golden_input(s)
      blocks = [g['band_%d_%d' % (s, b)] for b in range(case.WORKERS)]
      assert case.same(cc.find_centers(blocks, t1, t2, case.CF), g['centers_%d' % s])
    assert cc.find_centers([], 0.1, 0.1, 1).shape == (0, 0)
    assert cc.find_centers([np.zeros((0, 3))], 0.1, 0.1, 1).shape == (0, 3)
  finally:
    sp.shutdown()


@pytest.mark.parametrize('workers', (1, 4))
@pytest.mark.parametrize('backend', BACKENDS)
def test_column_split_points_are_retiled_and_float32_runs_in_float32(backend, workers):
  x, t1, t2 = case.golden_input(1)
  g = case.golden()
  _start(backend, workers)
  try:
    chains = case.WORKERS // workers
    # tiles of one or two columns: no tile holds whole rows
    split = expr.from_numpy(x, tile_hint=(case.ROWS, 2))
    labels, centers = cc.canopy_cluster(split, t1, t2, case.CF, chains_per_tile=chains, return_centers=True)
    assert case.same(centers, g['centers_1']) and case.same(np.asarray(labels.glom()), g['labels_1'])
    # float32 points: the NumPy bodies' float32 bytes, nothing converted to float64
    x32 = x.astype(np.float32)
    labels, centers = cc.canopy_cluster(x32, t1, t2, case.CF, chains_per_tile=chains, return_centers=True)
    blocks = [c[n > case.CF] for c, n, _ in (_canopy.canopy_numpy(x32[lo:hi], t1, t2) for lo, hi in case.bands())]
    c32, n32, _ = _canopy.canopy_numpy(np.concatenate(blocks), t1, t2)
    assert centers.dtype == np.float32 and case.same(centers, c32[n32 > case.CF])
    assert case.same(np.asarray(labels.glom()), _canopy.pdf_label_numpy(x32, centers))
    # integer points are converted to float64
    xi = np.round(x * 4).astype(np.int64)
    labels, centers = cc.canopy_cluster(xi, 1.5, 0.5, 0, chains_per_tile=chains, return_centers=True)
    assert centers.dtype == np.float64 and len(centers) >= 2
    assert case.same(np.asarray(labels.glom()), _canopy.pdf_label_numpy(xi.astype(np.float64), centers))
  finally:
    sp.shutdown()


@pytest.mark.parametrize('backend', BACKENDS)
def test_the_labels_are_lazy_and_no_centre_gives_minus_one(backend):
  x, t1, t2 = case.golden_input(0)
  _start(backend, 4)
  try:
    asked, body = [], _canopy.pdf_label

    def watched(xt, centers):
      asked.append(tuple(xt.shape))
      return body(xt, centers)
    _canopy.pdf_label = watched
    try:
      labels, centers = cc.canopy_cluster(x, t1, t2, case.CF, return_centers=True)
      assert isinstance(labels, expr.Expr) and asked == []        # nothing of the labels has run
      got = np.asarray(labels.force().glom())
      assert asked == [(case.ROWS // 4, x.shape[1])] * 4          # one tile body per band
      assert case.same(got, case.golden()['labels_0'])
      # cf above every count: no centre at all
      labels, centers = cc.canopy_cluster(x, t1, t2, case.ROWS, return_centers=True)
      assert centers.shape == (0, x.shape[1]) and centers.dtype == np.float64
      got = np.asarray(labels.glom())
      assert got.dtype == np.int32 and got.tolist() == [-1] * case.ROWS
    finally:
      _canopy.pdf_label = body
    for bad in (x.reshape(-1), x.reshape(4, 40, 3)):
      with pytest.raises(ValueError, match=r'\(n, d\)'):
        cc.canopy_cluster(bad, t1, t2)
    with pytest.raises(TypeError, match='real'):
      cc.canopy_cluster(x.astype(np.complex128), t1, t2)
    with pytest.raises(ValueError, match='chains'):
      cc.canopy_cluster(x, t1, t2, chains_per_tile=0)
    with pytest.raises(ValueError, match='t1'):
      cc.canopy_cluster(x, float('nan'), t2)
  finally:
    sp.shutdown()
