"""Integer-array indexing `x[idx]` (expr/filter.py) on the NumPy oracle backend, and the cases of
tests/gather_cases.py themselves; tests/test_gather_gpu.py runs the same operator cases on HipBackend."""
import numpy as np
import pytest

import spartan_amd as sp
from oracle.np_backend import NumpyBackend
from tests import gather_cases as gc


def test_cases_are_what_they_claim():
  assert [rb for rb, _, _ in gc.KERNEL_ROWS] == [1, 3, 2, 6, 4, 12, 16, 48, 2068]
  for rb, dtype, row in gc.KERNEL_ROWS:
    x = gc.source(gc.N_SRC, dtype, row)
    assert gc.row_bytes(x) == rb and x.shape[0] == gc.N_SRC
    assert len(set(r.tobytes() for r in x)) > gc.N_SRC // 2 or rb < 2          # rows differ: a wrong row shows
  idx = gc.INDEX
  assert idx.min() == -(gc.N_SRC - 1) and idx.max() == gc.N_SRC - 1            # every index but -N_SRC is used
  assert (idx < 0).any() and len(set(idx.tolist())) < len(idx) and (np.diff(idx) < 0).any()
  n_idx, n_src, words = gc.BIG
  assert (n_idx * words + 255) // 256 > 8192
  big = gc.big_index()
  assert big.min() > -n_src and big.max() < n_src and (big < 0).any()
  for bad in gc.OUT_OF_RANGE:
    assert any(i < -10 or i >= 10 for i in bad)


@pytest.mark.parametrize('workers', gc.OP_WORKERS)
def test_operator_on_the_numpy_backend(workers):
  sp.initialize(backend=NumpyBackend(), num_workers=workers)
  try:
    gc.run_operator_cases(sp)
  finally:
    sp.shutdown()


@pytest.mark.parametrize('workers', (1, 3))
def test_an_index_out_of_range_is_an_index_error_on_the_numpy_backend(workers):
  ctx = sp.initialize(backend=NumpyBackend(), num_workers=workers)
  try:
    gc.run_range_checks(sp, ctx.backend)
  finally:
    sp.shutdown()
