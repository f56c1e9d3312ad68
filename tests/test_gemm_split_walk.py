"""The order in which the split tier's mainloop hands out its 256 x 256 tiles (sp_gemm_split_tile_of_block in
spartan_amd/csrc/gemm_split.hpp), read on the host through sp_gemm_split_walk, which calls the function the kernel
compiles.  Two properties, no device:

  1. it is a bijection from block ids onto tiles for every grid -- a tile nobody takes is an unwritten block of C, a
     tile taken twice is written twice (and an `accumulate` adds twice);
  2. the 32 tiles that are resident on one XCD together (blocks b, b + 8, ...: consecutive local ids b >> 3, 32 CUs per
     XCD, one workgroup per CU) form the window the kernel's notes claim.  A workgroup loads one A panel (its tile row)
     and one B panel (its tile column) per k-tile, so what the XCD's L2 must fetch from beyond it for 32 tiles' worth of
     loads is the number of distinct tile rows plus distinct tile columns among them: 32 / RW + 32 / RH at least, and
     no window of 32 tiles has fewer than 4 + 8 = 12.  The walk of the fp32 kernels (sp_gemm_tile_of_block with
     GROUP_M = 2, which this kernel used before), restated below in Python, gives 2 + 16 = 18."""
import ctypes

import numpy as np
import pytest

from spartan_amd import _hip

WINDOW = (4, 8)                  # RH x RW: tile rows x tile columns of the landed window
PARENT_GROUP_M = 2


def _walk(tiles_m, tiles_n):
  n = tiles_m * tiles_n
  tm, tn = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
  p32 = ctypes.POINTER(ctypes.c_int32)
  assert _hip.lib().sp_gemm_split_walk(tiles_m, tiles_n, tm.ctypes.data_as(p32), tn.ctypes.data_as(p32)) == n
  return tm, tn


def _parent_walk(tiles_m, tiles_n):
  """sp_gemm_tile_of_block of gemm.hip: a contiguous range of the tile order per XCD; the order is m-fastest inside
  groups of GROUP_M tile rows, the last group clipped."""
  n = tiles_m * tiles_n
  g = PARENT_GROUP_M
  tm, tn = np.empty(n, np.int32), np.empty(n, np.int32)
  q, r = n >> 3, n & 7
  for b in range(n):
    xcd, local = b & 7, b >> 3
    t = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + local
    group = t // (g * tiles_n)
    first = group * g
    gsize = min(g, tiles_m - first)
    in_group = t - group * g * tiles_n
    tm[b], tn[b] = first + in_group % gsize, in_group // gsize
  return tm, tn


def _panels(tm, tn):
  """Distinct tile rows + distinct tile columns of every aligned run of 32 local ids of every XCD."""
  out = []
  for xcd in range(8):
    rows, cols = tm[xcd::8], tn[xcd::8]
    for s in range(0, rows.size, 32):
      out.append(np.unique(rows[s:s + 32]).size + np.unique(cols[s:s + 32]).size)
  return out


def _assert_bijection(tiles_m, tiles_n):
  tm, tn = _walk(tiles_m, tiles_n)
  assert tm.min() >= 0 and tm.max() < tiles_m and tn.min() >= 0 and tn.max() < tiles_n, (tiles_m, tiles_n)
  seen = np.bincount(tm.astype(np.int64) * tiles_n + tn, minlength=tiles_m * tiles_n)
  assert np.all(seen == 1), (tiles_m, tiles_n, np.flatnonzero(seen != 1)[:8])


def test_bijection_every_grid_up_to_48_by_48():
  for tiles_m in range(1, 49):
    for tiles_n in range(1, 49):
      _assert_bijection(tiles_m, tiles_n)


@pytest.mark.parametrize('grid', [(128, 16), (16, 128), (128, 32), (1, 2048), (2048, 1), (127, 33)])
def test_bijection_large_and_narrow_grids(grid):
  _assert_bijection(*grid)


def test_no_grid_no_walk():
  p32 = ctypes.POINTER(ctypes.c_int32)
  one = np.zeros(1, np.int32)
  for grid in ((0, 4), (4, 0), (-1, 4), (65536, 32768)):
    assert _hip.lib().sp_gemm_split_walk(grid[0], grid[1], one.ctypes.data_as(p32), one.ctypes.data_as(p32)) == 0


def test_the_restated_parent_walk_is_the_2_by_16_window():
  assert set(_panels(*_parent_walk(32, 32))) == {18}


def test_window_at_the_headline_grid():
  """8192^3: 32 x 32 tiles, 128 per XCD, four rounds of 32."""
  panels = _panels(*_walk(32, 32))
  assert len(panels) == 8 * 4
  assert set(panels) == {WINDOW[0] + WINDOW[1]}
  if WINDOW != (PARENT_GROUP_M, 32 // PARENT_GROUP_M):
    assert max(panels) < 18


@pytest.mark.parametrize('grid', [(128, 16), (128, 32), (31, 33)])
def test_window_no_wider_than_the_parents(grid):
  """(128, 16) and (128, 32): the K-split pipeline's outlines; (31, 33): clipped groups and ranges that straddle them."""
  ours, parents = max(_panels(*_walk(*grid))), max(_panels(*_parent_walk(*grid)))
  print('%s: %d panels at most per 32 resident tiles, the parent %d' % (grid, ours, parents))
  assert ours <= parents
