"""The split tier's mainloop (sp_gemm_glds_kernel_bf16x3, spartan_amd/csrc/gemm_split.hpp) at the two ends of a tile's
k-loop.  The address of the requested k-tile is a running base per image that steps by a slab per k-tile, and the clamp
of the last two requests is two copies of the body whose bases stand on the last k-tile, chosen by the parity of the
count.  What can go wrong: a boundary k-tile taken from the wrong place (a base one slab off, the k-tile of a
neighbouring tile), a first or last k-tile dropped or taken twice, the wrong copy of the body for the count's parity,
and a block stored in the wrong place or under the wrong mask, with and without accumulate.

Outlines: E1 (7681, 8196), 1023 tiles, the last ones one row and four columns wide, and E2 (7969, 8188), 1024 tiles:
four rounds of one workgroup per CU.  K is K0, K0 + 16 and K0 + 21, K0 the smallest multiple of 16 the plan
takes (asked of the plan): both parities of the k-tile count, which end in different copies of the body, and a partial
last k-tile.

  1. boundary k-tiles alone: A[i, k] = 1 + (7 i + 3 k) % 64 and B[k, j] = 1 + (5 j + 11 k) % 64 for k in S, zero
     elsewhere, S in turn the first k-tile, the second, the last but one and the last.  C[i, j] is an exact integer
     below 2^17 that depends on i and j through those k-tiles only: a k-tile taken from a neighbouring tile or one
     slab off changes it.  C is NaN-filled before the call;
  2. the same with accumulate onto C0[i, j] = (i + 3 j) % 1024, S the first and the last k-tile;
  3. dense: every k non-zero, same formulas, K0 and K0 + 21, through images cut beforehand and not, twice each into
     fresh NaN-filled buffers, lda, ldb and ldc padded;
  4. one round of tiles: a 4096 x 4096 x K shape (exactly 256 tiles, one per CU) the plan takes, if there is one (today
     there is none and the case skips);
  5. window flag: an element of 2^50 in one operand -- the kernel returns at once and the gated fp32 kernel gives the
     fp32 tier's bits (SP_GEMM_SPLIT=0 in a child process).

Every comparison is bit equality.  Expected values are int64 products on the host: A[i, :] depends on i through
(7 i) % 64 and B[:, j] on j through (5 j) % 64, so the product over S is a 64 x |S| x 64 int64 product, gathered by
those classes (checked against the direct int64 product on a stride of rows).  Each case first asserts that the plan
takes the split tier."""
import functools
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from spartan_amd import _hip  # noqa: E402
from tests import gemm_split_child as child  # noqa: E402
from tests import test_gemm_split_edges_gpu as edges  # noqa: E402

OUTLINES = {'E1': (7681, 8196), 'E2': (7969, 8188)}
OFFSETS = (0, 16, 21)
WHICH = ('first', 'second', 'last_but_one', 'last')
TILE = 256
WORKGROUPS = 256                 # GsCfg::SLOTS: the workgroups resident at a time, one per CU
I64 = np.int64


def _takes(m, n, k):
  return _hip.lib().sp_gemm_split_workspace_bytes(_hip.SP_F32, m, n, k) != 0


@functools.lru_cache(maxsize=None)
def _k0(name):
  m, n = OUTLINES[name]
  for k in range(16, 1 << 16, 16):
    if _takes(m, n, k):
      return k
  raise AssertionError('the plan never takes the split tier at %s' % (OUTLINES[name],))


def _pads(k):
  """Paddings of lda, ldb, ldc: lda and ldb multiples of 4 (the tier's precondition), all three non-zero."""
  return ((-k) % 4 + 4, 4, 12)


def _bits(x):
  return np.ascontiguousarray(x).view(np.uint32)


def _ktile(k, which):
  """The k of k-tile `which` of a K-long loop (the last one may be partial)."""
  kt = (k + 15) // 16
  t = {'first': 0, 'second': 1, 'last_but_one': kt - 2, 'last': kt - 1}[which]
  assert kt >= 4
  return np.arange(16 * t, min(16 * t + 16, k))


def _operands(m, n, k, ks):
  """A, B by the formulas at the k in `ks`, zero elsewhere, and the exact int64 product."""
  ks = np.asarray(ks, I64)
  i, j = np.arange(m, dtype=I64), np.arange(n, dtype=I64)
  a = np.zeros((m, k), np.float32)
  b = np.zeros((k, n), np.float32)
  a[:, ks] = 1 + (7 * i[:, None] + 3 * ks[None, :]) % 64
  b[ks, :] = 1 + (5 * j[None, :] + 11 * ks[:, None]) % 64
  r = np.arange(64, dtype=I64)
  small = (1 + (r[:, None] + 3 * ks[None, :]) % 64).dot(1 + (r[None, :] + 11 * ks[:, None]) % 64)   # int64, 64 x 64
  want = small[(7 * i) % 64][:, (5 * j) % 64]
  rows = np.arange(0, m, 997)
  assert np.array_equal(a[rows][:, ks].astype(I64).dot(b[ks].astype(I64)), want[rows])
  return a, b, want


def _nan_c(m, n, pad):
  from spartan_amd import devarray as D
  ld = n + pad
  return D.full((m * ld,), np.nan, np.float32).reshape(m, ld)[:, :n]


def _gemm(da, db, c0=None, prepared=None):
  """a . b (+ c0) on the split tier into a fresh buffer (NaN-filled where it does not accumulate), as a host array."""
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  (m, k), n = da.shape, db.shape[1]
  assert _takes(m, n, k), (m, n, k)
  c = _nan_c(m, n, _pads(k)[2]) if c0 is None else child.padded(c0, _pads(k)[2])
  kw = {'prepared_a': prepared[0], 'prepared_b': prepared[1]} if prepared else {}
  before = _hip.lib().sp_gemm_cut_launches()
  kernels.gemm_f32(da, db, c, accumulate=c0 is not None, **kw)
  assert _hip.lib().sp_gemm_cut_launches() - before == (0 if prepared else 2)
  D.synchronize()
  return c.numpy()


def _explain(got, want):
  """Bit equality with the exact integers `want`; on failure, where in the tile grid."""
  want = want.astype(np.float32)
  bad = _bits(got) != _bits(want)
  if not bad.any():
    return
  rows, cols = np.flatnonzero(bad.any(axis=1)), np.flatnonzero(bad.any(axis=0))
  raise AssertionError('%d elements differ (%d NaN) in %d rows and %d columns; tile rows %s, tile columns %s; first rows '
                       '%s, first columns %s' % (bad.sum(), np.isnan(got).sum(), rows.size, cols.size,
                                                 np.unique(rows // TILE)[:16], np.unique(cols // TILE)[:16], rows[:8], cols[:8]))


@pytest.mark.parametrize('name', list(OUTLINES))
def test_outlines_take_several_rounds_of_tiles(name):
  m, n = OUTLINES[name]
  tiles = -(-m // TILE) * -(-n // TILE)
  assert tiles > 3 * WORKGROUPS
  assert {'E1': tiles == 1023 and (m % TILE, n % TILE) == (1, 4), 'E2': tiles == 1024}[name]
  k0 = _k0(name)
  assert k0 % 16 == 0 and (k0 == 16 or not _takes(m, n, k0 - 16))
  for off in OFFSETS:
    assert _takes(m, n, k0 + off), off


# ---- 1., 2. boundary k-tiles alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', WHICH)
@pytest.mark.parametrize('off', OFFSETS)
@pytest.mark.parametrize('name', list(OUTLINES))
def test_boundary_ktile_alone(name, off, which):
  (m, n), k = OUTLINES[name], _k0(name) + off
  a, b, want = _operands(m, n, k, _ktile(k, which))
  assert 0 < want.min() and want.max() < 2 ** 17
  pads = _pads(k)
  _explain(_gemm(child.padded(a, pads[0]), child.padded(b, pads[1])), want)


@pytest.mark.parametrize('which', ('first', 'last'))
@pytest.mark.parametrize('off', OFFSETS)
@pytest.mark.parametrize('name', list(OUTLINES))
def test_boundary_ktile_alone_accumulates(name, off, which):
  (m, n), k = OUTLINES[name], _k0(name) + off
  a, b, want = _operands(m, n, k, _ktile(k, which))
  c0 = ((np.arange(m, dtype=I64)[:, None] + 3 * np.arange(n, dtype=I64)[None, :]) % 1024)
  assert (want + c0).max() < 2 ** 17 + 1024
  pads = _pads(k)
  _explain(_gemm(child.padded(a, pads[0]), child.padded(b, pads[1]), c0.astype(np.float32)), want + c0)


# ---- 3. dense ---------------------------------------------------------------------------------------------------------------
def _dense_twice(m, n, k, prepared):
  from spartan_amd import kernels
  a, b, want = _operands(m, n, k, np.arange(k))
  assert want.max() < 2 ** 24
  pads = _pads(k)
  da, db = child.padded(a, pads[0]), child.padded(b, pads[1])
  images = (kernels.gemm_prepare(da, 0), kernels.gemm_prepare(db, 1)) if prepared else None
  first = _gemm(da, db, prepared=images)
  second = _gemm(da, db, prepared=images)
  assert np.array_equal(_bits(first), _bits(second))
  _explain(first, want)


@pytest.mark.parametrize('prepared', [False, True])
@pytest.mark.parametrize('off', (0, 21))
@pytest.mark.parametrize('name', list(OUTLINES))
def test_dense_twice(name, off, prepared):
  m, n = OUTLINES[name]
  _dense_twice(m, n, _k0(name) + off, prepared)


# ---- 4. one tile per workgroup ----------------------------------------------------------------------------------------------
def test_one_tile_per_workgroup():
  m = n = 4096
  assert (m // TILE) * (n // TILE) == WORKGROUPS
  for k in range(16, 8192 + 1, 16):
    if _takes(m, n, k):
      break
  else:
    pytest.skip('the plan takes no 4096 x 4096 x K, K a multiple of 16 up to 8192: no shape with exactly %d tiles' % WORKGROUPS)
  a, b, want = _operands(m, n, k, np.arange(k))
  assert want.max() < 2 ** 24
  pads = _pads(k)
  da, db = child.padded(a, pads[0]), child.padded(b, pads[1])
  first, second = _gemm(da, db), _gemm(da, db)
  assert np.array_equal(_bits(first), _bits(second))
  _explain(first, want)


# ---- 5. window flag ---------------------------------------------------------------------------------------------------------
def test_window_flag_gives_the_fp32_tiers_bits():
  (m, n), k = OUTLINES['E1'], _k0('E1')
  assert _takes(m, n, k)
  a, b, _ = _operands(m, n, k, np.arange(k))
  a[m - 1, k - 1] = 2.0 ** 50            # in the one-row tiles at the lower edge
  pads = _pads(k)
  c0 = np.full((m, n), np.nan, np.float32)
  got = child.run(a, b, c0, pads, False)
  with tempfile.TemporaryDirectory() as tmp:
    want = edges._fp32_tier(a, b, np.zeros((m, n), np.float32), pads, False, tmp, 'tilestream')
  assert not np.isnan(got).any()
  assert np.array_equal(_bits(got), _bits(want))
