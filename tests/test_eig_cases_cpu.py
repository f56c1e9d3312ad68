"""The yardstick of the eigensolver tests, checked without a device: the tournament pairing, the NumPy transcription
(tests/eig_cases.jacobi) against the figures the issue gives for it and against its recorded run
(tests/golden/eig_yardstick.json), and the host fallback of examples/_dense.syev."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples import _dense
from tests import eig_cases as ec

DTYPES = (np.float32, np.float64)


@pytest.mark.parametrize('n', (1, 2, 3, 8, 9, 64, 65))
def test_every_pair_meets_once_per_sweep(n):
  m = n + (n & 1)
  seen = set()
  for r in range(m - 1):
    p, q = ec.round_pairs(n, r)
    assert len(p) == n // 2 and np.all(p < q) and np.all(q < n)
    assert len(set(p.tolist()) | set(q.tolist())) == 2 * len(p)              # disjoint within the round
    seen |= set(zip(p.tolist(), q.tolist()))
  assert len(seen) == n * (n - 1) // 2


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('kind', ec.KINDS)
def test_the_transcription_at_65_is_the_recorded_one_and_in_the_stated_range(kind, dtype):
  """The issue's table for the transcription at n = 65: fp32 6-9 sweeps, resid 2.2-2.4, orth 18-21, eigs 2.5-3.3; fp64
  8-19 sweeps, resid 1.3-3.6, orth 10-31, eigs 1.3-4.5 (here within a factor 1.5 of those ranges: the stored inputs
  differ in their last bits between LAPACK builds).  The recorded figures are this transcription's, to 25 %."""
  live = ec.yardstick(kind, 65, dtype, live=True)
  rec = ec.yardstick(kind, 65, dtype)
  print('transcription %s n=65 %s: resid %.3g orth %.3g eigs %.3g sweeps %d (recorded %s)'
        % (kind, np.dtype(dtype).name, live[0], live[1], live[2], live[3], ['%.3g' % v for v in rec]))
  lo, hi = ((2.2, 18, 2.5, 6), (2.4, 21, 3.3, 9)) if np.dtype(dtype) == np.float32 else ((1.3, 10, 1.3, 8), (3.6, 31, 4.5, 19))
  for v, a, b in zip(live, lo, hi):
    assert a / 1.5 <= v <= b * 1.5
  np.testing.assert_allclose(live[:3], rec[:3], rtol=0.25)
  assert abs(live[3] - rec[3]) <= 1


def test_every_input_of_the_gpu_tests_has_a_recorded_yardstick():
  from tests.golden.make_golden_eig import CASES
  for dtype in DTYPES:
    for kind, n in CASES:
      rec = ec.recorded()[ec.key(kind, n, dtype)]
      assert len(rec) == 4 and rec[3] <= 26 and all(np.isfinite(rec))


def test_the_eig_header_the_binding_and_the_library_agree():
  import ctypes
  import os
  from spartan_amd import _hip
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  names = _declared_functions(os.path.join(ROOT, 'include', 'spartan_hip_eig.h'))
  assert names == sorted(_hip.EXPORTS_EIG) == ['sp_syevj', 'sp_syevj_workspace_bytes']
  assert not set(names) & set(_declared_functions(EXTRAS_HEADER)) and not set(names) & set(_hip.EXPORTS)
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  x = _hip.extras()                                   # host code: sizes need no device
  assert x.sp_syevj_workspace_bytes(_hip.SP_F32, 0) > 0
  assert x.sp_syevj_workspace_bytes(_hip.SP_F64, 257) >= 4 * 257 * 257 * 8


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_dense_syev_falls_back_to_lapack_on_the_numpy_backend(dtype):
  from oracle.np_backend import NumpyBackend
  a = ec.matrix('pm', 65, dtype)
  dirty = np.tril(a) + np.triu(np.full(a.shape, np.nan, dtype), 1)          # the lower triangle is read
  sp.initialize(backend=NumpyBackend(), num_workers=1)
  try:
    w, v = _dense.syev(dirty)
    with pytest.raises(ValueError):
      _dense.syev(np.ones((3, 4), dtype))
  finally:
    sp.shutdown()
  assert w.dtype == np.dtype(dtype) and v.dtype == np.dtype(dtype) and np.all(w[1:] >= w[:-1])
  ec.check('lapack syevd pm n=65 %s' % np.dtype(dtype).name, a, w, v, ec.yardstick('pm', 65, dtype))
