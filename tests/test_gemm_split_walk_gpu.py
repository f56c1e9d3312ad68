"""The split tier's tile walk (sp_gemm_split_tile_of_block, spartan_amd/csrc/gemm_split.hpp) on the device: every
256 x 256 tile of C is written, and written once, on grids the walk has to clip -- tile counts that are no multiple of
8 (the XCDs' ranges differ in length) or of 32, a ragged last tile row and column, more than one round of 256
workgroups, and the tall outline of the K-split pipeline.  tests/test_gemm_split_walk.py shows the bijection on the
host; here the kernel itself takes the function's answer.

Integer-valued operands by the recipe of tests/test_gemm_split_gpu.py, so the float64 product is exact and the result
must have its bits:
  * accumulate=False into a C that is NaN everywhere: a tile nobody took keeps its NaN;
  * accumulate=True onto a random integer C: a tile taken twice adds its product twice.
Integer data has the same bits on the fp32 tier, so every case asserts first that the plan takes the split tier
(sp_gemm_split_workspace_bytes is non-zero).  Each K is the smallest multiple of 16 at which the built library's plan
takes the tier at its outline (asked of the library: 592, 592, 192, 304), so the k-loops are as short as they get."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from spartan_amd import _hip  # noqa: E402
from tests import gemm_split_child as child  # noqa: E402

SHAPES = {                                 # (M, N, K): the tile grid
    'ragged_19x53': (4609, 13316, 592),    # 1007 tiles = 7 mod 8; one valid row and four valid columns in the last tiles
    'ragged_53x19': (13313, 4612, 592),
    'two_rounds_62x33': (15617, 8196, 192),   # 2046 tiles
    'ksplit_128x16': (32513, 3844, 304),   # the K-split pipeline's outline
}
PADS = (4, 4, 12)


@functools.lru_cache(maxsize=1)
def _case(name):
  m, n, k = SHAPES[name]
  rng = np.random.RandomState(20261021)
  a = rng.randint(-3, 4, size=(m, k)).astype(np.float32)
  b = rng.randint(-3, 4, size=(k, n)).astype(np.float32)
  a[:, 5] = rng.randint(-(1 << 18), 1 << 18, size=m)           # a few wide ones: all three pieces of an operand at work
  b[7, :] = rng.randint(-255, 256, size=n)
  c0 = rng.randint(-9, 10, size=(m, n)).astype(np.float32)
  prod = a.astype(np.float64).dot(b.astype(np.float64))
  assert np.abs(prod).max() + 9 < 2 ** 24
  for x in (a, b, c0, prod):
    x.setflags(write=False)
  return a, b, c0, prod


def _explain(got, want):
  """Bit equality; on failure, which tiles differ and how."""
  bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
  if not bad.any():
    return
  rows, cols = np.nonzero(bad)
  tiles = sorted(set(zip((rows // 256).tolist(), (cols // 256).tolist())))
  raise AssertionError('%d elements differ (%d of them NaN) in %d tiles; the first: %s'
                       % (bad.sum(), np.isnan(got[bad]).sum(), len(tiles), tiles[:12]))


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('name', list(SHAPES))
def test_every_tile_written_once(name, accumulate):
  m, n, k = SHAPES[name]
  assert _hip.lib().sp_gemm_split_workspace_bytes(_hip.SP_F32, m, n, k) != 0, SHAPES[name]
  a, b, c0, prod = _case(name)
  if accumulate:
    got = child.run(a, b, c0, PADS, True)
    want = (prod + c0).astype(np.float32)
  else:
    got = child.run(a, b, np.full((m, n), np.nan, np.float32), PADS, False)
    want = prod.astype(np.float32)
  _explain(got, want)
