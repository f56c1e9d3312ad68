"""What the fuzzy k-means tests stand on, without a GPU: the recipe and the NumPy tile body of the driver
(examples/_fuzzy.py) against the oracle and the derived bound of tests/fuzzy_cases.py, the body against the reference's
recorded mappers (tests/golden/fuzzy_w4.npz), and the agreement of header, binding and library."""
import ctypes
import os

import numpy as np
import pytest

from spartan_amd import _hip
from tests import fuzzy_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = (np.float32, np.float64)
# the (n, k, d, m) at which the bound was checked when it was derived, and the edges of the kernel's tiling
SHAPES = ((130, 70, 20, 2.0), (65, 3, 257, 2.0), (200, 129, 5, 1.5), (100, 64, 33, 3.0), (1000, 17, 64, 2.0))


def _start():
  import spartan_amd as sp
  from oracle.np_backend import NumpyBackend
  sp.initialize(backend=NumpyBackend(), num_workers=1)
  return sp


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d-m%g' % s)
def test_the_numpy_tile_body_meets_the_bound_at_the_shapes_of_its_derivation(shape, dtype):
  from spartan_amd.examples import _fuzzy
  n, k, d, m = shape
  x, c = fc.case(n, k, d, np.dtype(dtype))
  want = fc.oracle_of_case(n, k, d, np.dtype(dtype), m)
  labels, sums, wsum, u = _fuzzy.step_numpy(x, c, m, want_u=True)
  share = fc.check_step(x, c, m, labels, sums, wsum, u, want=want, label='numpy body %s %s' % (shape, np.dtype(dtype).name))
  assert share < 0.1                     # (what the derivation found: a restatement this close has no dropped term)
  assert labels.tobytes() == np.asarray(want['labels'], np.int64).tobytes()
  assert np.all(np.isfinite(u)) and not np.any(labels == k - 1)       # the planted zero distance; the duplicate centre


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('m', fc.MS)
def test_the_tile_body_on_the_numpy_backend(m, dtype):
  from spartan_amd.examples import _fuzzy
  sp = _start()
  try:
    for n, k, d in ((130, 70, 20), (7, 1, 3), (64, 5, 0), (0, 4, 6), (40, 65, 17)):
      x, c = fc.case(n, k, d, np.dtype(dtype))
      out = _fuzzy.fuzzy_step(x, c, m, want_u=True)
      assert len(out) == 4 and len(_fuzzy.fuzzy_step(x, c, m)) == 3
      fc.check_step(x, c, m, *out, label='numpy backend %s m=%g %s' % ((n, k, d), m, np.dtype(dtype).name))
      if d == 0:
        assert np.all(np.abs(out[3] - 1.0 / k) <= fc.eps(n, k, d, m, dtype)['u'] / k) and not np.any(out[0])
      if n == 0:
        assert not np.any(out[1]) and not np.any(out[2])
    x, c = fc.case(130, 70, 20, np.dtype(dtype))
    with pytest.raises(TypeError, match='astype'):
      _fuzzy.fuzzy_step(x.astype(np.int32), c, m)
    with pytest.raises(TypeError, match='astype'):
      _fuzzy.fuzzy_step(x, c.astype(np.float16), m)
    with pytest.raises(TypeError, match='astype'):
      _fuzzy.fuzzy_step(x.astype(np.float32), c.astype(np.float64), m)
    for bad in (1.0, 0.5, float('nan'), float('inf')):
      with pytest.raises(ValueError, match='m = '):
        _fuzzy.fuzzy_step(x, c, bad)
    with pytest.raises(ValueError, match='k = 0'):
      _fuzzy.fuzzy_step(x, c[:0], m)
    with pytest.raises(ValueError, match='do not fit'):
      _fuzzy.fuzzy_step(x, c[:, :19], m)
  finally:
    sp.shutdown()


def test_a_nan_row_in_the_numpy_body():
  from spartan_amd.examples import _fuzzy
  x, c = fc.case(130, 70, 20, np.dtype(np.float64), nan_row=True)
  clean, _ = fc.case(130, 70, 20, np.dtype(np.float64))
  labels, sums, wsum, u = _fuzzy.step_numpy(x, c, 2.0, want_u=True)
  base = _fuzzy.step_numpy(clean, c, 2.0, want_u=True)
  assert labels[5] == 0 and np.all(np.isnan(u[5])) and np.all(np.isnan(sums)) and np.all(np.isnan(wsum))
  assert np.delete(u, 5, axis=0).tobytes() == np.delete(base[3], 5, axis=0).tobytes()
  assert np.delete(labels, 5).tobytes() == np.delete(base[0], 5).tobytes()


@pytest.mark.parametrize('m', (2.0, 1.5))
def test_the_numpy_body_equals_the_reference_mappers(m):
  """tests/golden/fuzzy_w4.npz: the reference's two mappers chained for two iterations (float64, cdist)."""
  from spartan_amd.examples import _fuzzy
  g = np.load(os.path.join(HERE, 'golden', 'fuzzy_w4.npz'))
  x, centers = g['points'], g['centers0']
  tag = 'm%g_' % m
  for it in ('1', '2'):
    labels, sums, wsum, u = _fuzzy.step_numpy(x, centers, m, want_u=True)
    centers = sums / wsum[:, None]
    for name, got in (('fuzzy', u), ('centers', centers)):
      want = g[tag + name + it]
      err = float(np.max(np.abs(got - want) / np.abs(want)))
      print('m = %g, iteration %s: %s differs from the reference by %.3g relative' % (m, it, name, err))
      assert err <= 1e-12
    assert labels.tobytes() == g[tag + 'labels' + it].astype(np.int64).tobytes()


def test_the_fuzzy_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  header = os.path.join(ROOT, 'include', 'spartan_hip_fuzzy.h')
  names = _declared_functions(header)
  assert names == sorted(_hip.EXPORTS_FUZZY) == ['sp_fuzzy_step', 'sp_fuzzy_step_workspace_bytes']
  others = (set(_hip.EXPORTS) | set(_hip.EXPORTS_EXTRAS) | set(_hip.EXPORTS_EIG) | set(_hip.EXPORTS_KNN)
            | set(_hip.EXPORTS_GRAPH) | set(_hip.EXPORTS_ALS))
  for h in (EXTRAS_HEADER,) + tuple(os.path.join(ROOT, 'include', 'spartan_hip_%s.h' % s) for s in ('eig', 'knn', 'graph', 'als')):
    others |= set(_declared_functions(h))
  assert not set(names) & others
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  x = _hip.extras()                                   # host code: sizes need no device
  f32, f64 = _hip.SP_F32, _hip.SP_F64
  size = x.sp_fuzzy_step_workspace_bytes
  assert size(f32, 0, 4, 6, 0) == 256 == size(f32, 64, 4, 6, 7)                 # z alone: one block of rows is one range
  assert size(f64, 300, 70, 20, 1) == 2560                                      # 300 z of 8 bytes, rounded up to 256
  partials = -(-3 * 70 * 20 * 8 // 256) * 256                                  # three partial [k, d], rounded up to 256
  assert size(f64, 300, 70, 20, 3) == 2560 + partials + 3 * 70 * 8              # ... and three partial [k]
  assert size(f64, 300, 70, 20, 7) == size(f64, 300, 70, 20, 5)                 # at most ceil(300 / 64) = 5 ranges
  assert size(f32, 300, 70, 20, 0) == size(f32, 300, 70, 20, 1)                 # few rows: the library does not cut them
  assert size(_hip.SP_I32, 300, 70, 20, 0) == 0 == size(f32, 300, 0, 20, 0) == size(f32, -1, 4, 4, 0)
