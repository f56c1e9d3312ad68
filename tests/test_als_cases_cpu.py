"""What the ALS tests stand on, without a GPU: the oracle of tests/als_cases.py against scipy.linalg.lstsq (the
reference's solver), the NumPy tile body of the driver (examples/_als.py) against the derived bound, and the agreement
of header, binding and library."""
import ctypes
import os
import re

import numpy as np
import pytest

from spartan_amd import _hip
from tests import als_cases as ac

DTYPES = (np.float32, np.float64)
# the (m, n, f) of the bound's own check (als_cases: the restatement stays between 1e-4 and 0.13 of the bound)
SHAPES = ((5, 7, 1), (9, 65, 3), (8, 130, 20), (4, 1031, 20), (4, 300, 64), (3, 2049, 33))


@pytest.mark.parametrize('implicit', (False, True), ids=('explicit', 'implicit'))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_the_oracle_agrees_with_lstsq(shape, implicit):
  """Per row, the reference's own formulation (spartan/examples/als.py:7-46, restated) in float64: within float64
  rounding times kappa(A_i) of the oracle -- kappa (n + 2 + 64 f) u: A_i and b_i formed in float64 are off by
  gamma_{n+2} relative to their absolute sums (which here, all operands being non-negative, are A_i and b_i
  themselves), and 64 f u is allowed for the backward error of LAPACK's SVD solve."""
  from scipy.linalg import lstsq
  r, y = ac.case(*shape, dtype=np.float64)
  want, bound, kappa = ac.oracle_of_case(*shape, dtype=np.float64, implicit=implicit)
  f = y.shape[1]
  yty = y.T.dot(y)
  for i in range(r.shape[0]):
    if implicit:
      cu = r[i].reshape(-1, 1) * ac.ALPHA + 1
      a = yty + y.T.dot(y * (cu - 1)) + np.eye(f) * ac.LA
      b = (y * cu)[r[i] > 0].sum(axis=0)
    else:
      nz = r[i].nonzero()[0]
      a = y[nz].T.dot(y[nz]) + ac.LA * nz.shape[0] * np.eye(f)
      b = y[nz].T.dot(r[i, nz])
    got = lstsq(a, b)[0]
    err = float(ac.errors(got[None], want[i][None])[0])
    limit = max(kappa[i], 1.0) * (r.shape[1] + 2 + 64 * f) * ac.U[np.dtype(np.float64)]
    print('row %d: |lstsq - oracle| / |oracle| = %.3g (limit %.3g, kappa %.3g)' % (i, err, limit, kappa[i]))
    assert err <= limit


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('implicit', (False, True), ids=('explicit', 'implicit'))
def test_the_numpy_tile_body_meets_the_bound(implicit, dtype):
  import spartan_amd as sp
  from oracle.np_backend import NumpyBackend
  from spartan_amd.examples import _als
  sp.initialize(backend=NumpyBackend(), num_workers=1)
  try:
    for shape in SHAPES + ((3, 0, 4), (1, 1, 2)):
      r, y = ac.case(*shape, dtype=dtype)
      want, bound, _ = ac.oracle_of_case(*shape, dtype=dtype, implicit=implicit)
      info = np.zeros((1,), np.int32)
      got = _als.als_solve(r, y, ac.LA, ac.ALPHA, implicit, info=info)
      assert got.dtype == np.dtype(dtype) and got.shape == want.shape and info[0] == 0
      ac.check(got, want, bound, 'numpy body %s %s %s' % (shape, np.dtype(dtype).name, 'implicit' if implicit else 'explicit'))
      if not implicit and shape[0] > 1:
        assert not np.any(got[1])
    # negative ratings: fine in explicit mode, an indefinite system in implicit mode
    r, y = ac.case(6, 40, 5, dtype, negative=True)
    if not implicit:
      want, bound, _ = ac.oracle_of_case(6, 40, 5, dtype, False, negative=True)
      ac.check(_als.als_solve(r, y, ac.LA, ac.ALPHA, False), want, bound, 'numpy body, negative ratings')
    else:
      clean, y = ac.case(6, 40, 5, dtype)
      base = _als.als_solve(clean, y, ac.LA, ac.ALPHA, True)
      for poison in (-500.0, np.nan):
        bad = np.array(clean)
        bad[4, 7] = poison
        info = np.zeros((1,), np.int32)
        got = _als.als_solve(bad, y, ac.LA, ac.ALPHA, True, info=info)
        assert info[0] == 5 and np.all(np.isnan(got[4]))
        assert np.delete(got, 4, axis=0).tobytes() == np.delete(base, 4, axis=0).tobytes()
        got = _als.als_solve(clean, y, ac.LA, ac.ALPHA, True, info=info)     # a set word is left alone
        assert info[0] == 5 and got.tobytes() == base.tobytes()
    with pytest.raises(TypeError, match='astype'):
      _als.als_solve(r.astype(np.int32), y, ac.LA, ac.ALPHA, implicit)
    with pytest.raises(ValueError, match='64'):
      _als.als_solve(r, np.zeros((40, 65), dtype), ac.LA, ac.ALPHA, implicit)
  finally:
    sp.shutdown()


def test_the_als_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  header = os.path.join(ROOT, 'include', 'spartan_hip_als.h')
  names = _declared_functions(header)
  assert names == sorted(_hip.EXPORTS_ALS) == ['sp_als_solve', 'sp_als_solve_workspace_bytes']
  others = set(_hip.EXPORTS) | set(_hip.EXPORTS_EXTRAS) | set(_hip.EXPORTS_EIG) | set(_hip.EXPORTS_KNN) | set(_hip.EXPORTS_GRAPH)
  for h in (EXTRAS_HEADER, os.path.join(ROOT, 'include', 'spartan_hip_eig.h'), os.path.join(ROOT, 'include', 'spartan_hip_knn.h'),
            os.path.join(ROOT, 'include', 'spartan_hip_graph.h')):
    others |= set(_declared_functions(h))
  assert not set(names) & others
  assert int(re.search(r'#define\s+SP_ALS_MAX_F\s+(\d+)', open(header).read()).group(1)) == _hip.SP_ALS_MAX_F == 64
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  x = _hip.extras()                                   # host code: sizes need no device
  f32, f64 = _hip.SP_F32, _hip.SP_F64
  assert 0 < x.sp_als_solve_workspace_bytes(f32, 10, 100, 20, 0) <= 256             # the word of the failing row
  assert x.sp_als_solve_workspace_bytes(f64, 10, 1031, 20, 1) >= 256 + (1 + 5) * 20 * 20 * 8    # Y^T Y and 5 ranges of 256
  assert x.sp_als_solve_workspace_bytes(f32, 10, 100, 65, 0) == 0 == x.sp_als_solve_workspace_bytes(_hip.SP_I32, 10, 100, 20, 0)
