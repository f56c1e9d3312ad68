"""What the nearest-neighbour tests stand on, without a GPU: the derived bound of tests/knn_cases.py against three
summation orders of the difference form in NumPy, the NumPy tile bodies of the driver against the oracle, and the
agreement of header, binding and library."""
import ctypes
import os
import re

import numpy as np
import pytest

from spartan_amd import _hip
from tests import knn_cases as kc

DTYPES = (np.float32, np.float64)


def _orders(q, x):
  """d2 in the inputs' dtype, every operation rounded to it, summed forwards, backwards and pairwise."""
  terms = (q[:, None, :] - x[None, :, :]) ** 2
  fwd = np.zeros(terms.shape[:2], q.dtype)
  bwd = np.zeros(terms.shape[:2], q.dtype)
  for j in range(q.shape[1]):
    fwd = fwd + terms[:, :, j]
    bwd = bwd + terms[:, :, q.shape[1] - 1 - j]
  return fwd, bwd, terms.sum(axis=2)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('d', (1, 3, 33, 200))
def test_the_derived_bound_holds_in_three_summation_orders(d, dtype):
  q, x = kc.real_case(37, 257, d, dtype)
  exact = kc.exact_dist2(q, x)
  g = kc.gamma(d, dtype)
  for name, got in zip(('forward', 'backward', 'pairwise'), _orders(q, x)):
    err = np.abs(got.astype(np.longdouble) - exact)
    worst = float((err / np.where(exact > 0, g * exact, 1)).max())
    print('d=%d %s %s: max |computed - exact| / (gamma exact) = %.3g' % (d, np.dtype(dtype).name, name, worst))
    assert np.all(err <= g * exact)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_numpy_tile_bodies_match_the_oracle(dtype):
  import spartan_amd as sp
  from oracle.np_backend import NumpyBackend
  from spartan_amd.examples.sklearn.neighbors import _knn
  sp.initialize(backend=NumpyBackend(), num_workers=1)
  try:
    for nq, npts, d, k in ((5, 40, 3, 7), (3, 4, 33, 17), (2, 0, 3, 5), (4, 9, 0, 3)):
      q, x = kc.integer_case(nq, npts, d, dtype)
      dist2, idx = _knn.knn(q, x, k, index_offset=kc.BIG_OFFSET)
      kc.check_exact(dist2, idx, q, x, k, kc.BIG_OFFSET)
    q, x = kc.integer_case(6, 120, 3, dtype)
    parts = [_knn.knn(q, x[lo:lo + 40], 17, index_offset=lo) for lo in (0, 40, 80)]
    dist2, idx = _knn.knn_merge(np.concatenate([p[0] for p in parts], axis=1),
                                np.concatenate([p[1] for p in parts], axis=1), 17)
    kc.check_exact(dist2, idx, q, x, 17)
    x[7, 1] = np.nan
    dist2, idx = _knn.knn(q, x, 120)
    assert np.all(idx[:, -1] == -1) and np.all(np.isposinf(dist2[:, -1])) and not np.any(idx == 7)
  finally:
    sp.shutdown()


def test_the_knn_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  header = os.path.join(ROOT, 'include', 'spartan_hip_knn.h')
  names = _declared_functions(header)
  assert names == sorted(_hip.EXPORTS_KNN) == ['sp_knn', 'sp_knn_merge', 'sp_knn_workspace_bytes']
  assert not set(names) & set(_declared_functions(EXTRAS_HEADER)) and not set(names) & set(_hip.EXPORTS)
  assert int(re.search(r'#define\s+SP_KNN_MAX_K\s+(\d+)', open(header).read()).group(1)) == _hip.KNN_MAX_K == 128
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  x = _hip.extras()                                   # host code: sizes need no device
  f32 = _hip.SP_F32
  assert x.sp_knn_workspace_bytes(f32, 64, 1000, 8, 5, 1) == 0                     # one range: nothing to merge
  assert x.sp_knn_workspace_bytes(f32, 64, 1000, 8, 5, 3) >= 64 * 3 * 5 * (4 + 8)
  assert x.sp_knn_workspace_bytes(f32, 64, 2, 8, 5, 7) >= 64 * 2 * 5 * (4 + 8)       # min(splits, np) ranges
  assert x.sp_knn_workspace_bytes(f32, 64, 2, 8, 5, 7) < 64 * 3 * 5 * (4 + 8) + 256
  assert x.sp_knn_workspace_bytes(f32, 2, 8195, 3, 5, 0) > 0                       # the library's own cut
  assert x.sp_knn_workspace_bytes(f32, 2, 4000, 3, 5, 0) == 0
