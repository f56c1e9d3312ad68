"""The split tier's mainloop (sp_gemm_glds_kernel_bf16x3, spartan_amd/csrc/gemm_split.hpp) on 16x16x32 bf16 MFMAs: four
waves of 128 x 128 per 256 x 256 tile, 8 x 8 accumulator blocks of 16 x 16 per wave, and two piece products per MFMA --
lanes 0-31 of an operand hold the 16 k of one image, lanes 32-63 the same 16 k of another.  What can go wrong there is
the C/D map of a block, a block's, a wave's or a block parity's base address, a tail row or column stored or dropped,
and a half of a concatenated operand taken from the wrong image or the wrong 8-k chunk.  So, at the two outlines of
tests/test_gemm_split_edges_gpu.py whose tails cross full 16-blocks and end inside one (E2) and leave one valid row and
four valid columns in the last tiles (E1), and at the SHORTEST loops the plan lets through -- K0 is the smallest
multiple of 16 the tier takes at the outline, found by asking the plan --:

  1. block map: A[i, i % K] = 2^(i % 5), zero elsewhere, B dense odd integers below 2^20 that are a fixed function of
     (k, j): C[i, j] is ONE exact product that names its row, its column and its k.  K0 and K0 + 16, with and without
     accumulate, C filled with NaN where it does not accumulate;
  2. pairing: the six-term construction of tests/test_gemm_split_edges_gpu.py (classes hh hm mh mm / hh hm hl /
     hh mh lh of k % 3) at K0, the non-zero of A at k = i % K, which puts it in every one of the 16 k positions of the
     first and of the last k-tile (and of every other one);
  3. dense integers: that file's recipe at K0, K0 + 16 and K0 + 21, through images cut beforehand
     (kernels.gemm_prepare, both operands) and not, each product twice into fresh NaN-filled buffers.

Every comparison is bit equality: there is no tolerance.  Integer data has the same bits on the fp32 tier, so each case
asserts first that the plan takes the split tier (sp_gemm_split_workspace_bytes is non-zero)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from spartan_amd import _hip  # noqa: E402
from tests import gemm_split_child as child  # noqa: E402
from tests import test_gemm_split_edges_gpu as edges  # noqa: E402

OUTLINES = {'E2': (7969, 8188), 'E1': (7681, 8196)}
OFFSETS = (0, 16, 21)            # K - K0: both parities of the k-tile count, then K % 16 = 5 on a third count
F64 = np.float64


def _ws_bytes(name, k):
  m, n = OUTLINES[name]
  return _hip.lib().sp_gemm_split_workspace_bytes(_hip.SP_F32, m, n, k)


@functools.lru_cache(maxsize=None)
def _k0(name):
  """The smallest multiple of 16 at which the plan takes the split tier at the outline."""
  for k in range(16, 1 << 16, 16):
    if _ws_bytes(name, k) != 0:
      print('%s: K0 = %d (%d k-tiles)' % (name, k, k // 16))
      return k
  raise AssertionError('the plan never takes the split tier at %s' % (OUTLINES[name],))


def _pads(k):
  """Paddings of lda, ldb, ldc: lda and ldb multiples of 4 (the tier's precondition), all three non-zero."""
  return ((-k) % 4 + 4, 4, 12)


def _bits(x):
  return np.ascontiguousarray(x).view(np.uint32)


def _nan_c(m, n, pad):
  """A fresh C view, pitch n + pad, in a buffer that is NaN everywhere."""
  from spartan_amd import devarray as D
  ld = n + pad
  return D.full((m * ld,), np.nan, np.float32).reshape(m, ld)[:, :n]


def _gemm(name, da, db, c0=None, prepared=None):
  """a . b (+ c0) on the split tier into a fresh buffer, as a host array.  da, db: device views (child.padded);
  prepared: (gemm_prepare(da, 0), gemm_prepare(db, 1)) or None.  Unprepared, the call must launch two cut kernels; with
  both operands cut beforehand, none."""
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  (m, k), n = da.shape, db.shape[1]
  assert (m, n) == OUTLINES[name] and _ws_bytes(name, k) != 0, (name, k)
  c = _nan_c(m, n, _pads(k)[2]) if c0 is None else child.padded(c0, _pads(k)[2])
  kw = {'prepared_a': prepared[0], 'prepared_b': prepared[1]} if prepared else {}
  before = _hip.lib().sp_gemm_cut_launches()
  kernels.gemm_f32(da, db, c, accumulate=c0 is not None, **kw)
  assert _hip.lib().sp_gemm_cut_launches() - before == (0 if prepared else 2)
  D.synchronize()
  return c.numpy()


def _explain(got, want, ki=None):
  """Bit equality, and on failure where the differences lie in the tile, the wave tile and the 16 x 16 block."""
  bad = _bits(got) != _bits(want)
  if not bad.any():
    return
  rows, cols = np.flatnonzero(bad.any(axis=1)), np.flatnonzero(bad.any(axis=0))
  msg = '%d elements differ (%d NaN) in %d rows and %d columns; first rows %s, first columns %s; rows %% 16: %s; ' \
        'columns %% 16: %s; 16-blocks of the wave tile: rows %s, columns %s' % (
            bad.sum(), np.isnan(got).sum(), rows.size, cols.size, rows[:8], cols[:8], np.unique(rows % 16),
            np.unique(cols % 16), np.unique(rows % 128 // 16), np.unique(cols % 128 // 16))
  if ki is not None:
    msg += '; k %% 16 of the bad rows: %s, their k-tiles: %s' % (np.unique(ki[rows] % 16), np.unique(ki[rows] // 16)[:8])
  raise AssertionError(msg)


@pytest.mark.parametrize('name', list(OUTLINES))
def test_k0_is_the_shortest_loop_the_plan_allows(name):
  k0 = _k0(name)
  assert k0 % 16 == 0 and _ws_bytes(name, k0) != 0
  assert k0 == 16 or _ws_bytes(name, k0 - 16) == 0
  for off in OFFSETS:
    assert _ws_bytes(name, k0 + off) != 0, off
  m, n = OUTLINES[name]
  assert {'E2': (m % 256, n % 256) == (33, 252), 'E1': (m % 256, n % 256) == (1, 4)}[name]


# ---- 1. block map: one exact product per element, which names its row, column and k -------------------------------------
def _odd_below_2_20(k, n):
  """B[k, j]: an odd integer below 2^20, a fixed (hashed) function of (k, j)."""
  kk, jj = np.arange(k, dtype=np.uint64)[:, None], np.arange(n, dtype=np.uint64)[None, :]
  h = ((kk * np.uint64(8209) + jj) * np.uint64(2654435761)) & np.uint64(0xffffffff)
  return (((h >> np.uint64(13)) << np.uint64(1)) | np.uint64(1)).astype(np.float32)


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('off', OFFSETS[:2])
@pytest.mark.parametrize('name', list(OUTLINES))
def test_block_map_one_product_per_element(name, off, accumulate):
  (m, n), k = OUTLINES[name], _k0(name) + off
  ki = np.arange(m) % k
  av = (2.0 ** (np.arange(m) % 5)).astype(np.float32)
  a = np.zeros((m, k), np.float32)
  a[np.arange(m), ki] = av
  b = _odd_below_2_20(k, n)
  assert b.max() < 2 ** 20 and np.all(b % 2 == 1)
  want = av[:, None] * b[ki]                            # (a power of two up to 16 times 20 bits: exact, below 2^24 - 9)
  c0 = None
  if accumulate:
    c0 = ((np.arange(m)[:, None] * 7 + np.arange(n)[None, :]) % 19 - 9).astype(np.float32)
    want = want + c0                                    # (integers below 2^24: exact)
    assert np.abs(want).max() < 2 ** 24
  pads = _pads(k)
  got = _gemm(name, child.padded(a, pads[0]), child.padded(b, pads[1]), c0)
  _explain(got, want, ki)


# ---- 2. pairing: the six piece products, two per MFMA ---------------------------------------------------------------------
@pytest.mark.parametrize('name', list(OUTLINES))
def test_six_piece_products_pair_the_right_halves(name):
  (m, n), k = OUTLINES[name], _k0(name)
  for seed in range(20150708, 20150716):
    ki, av, b, _ = edges._draw(seed, m, n, k)
    if edges._terms_bite(ki, av, b):
      break
  else:
    raise AssertionError('no draw in which every named piece product is non-zero in 3/4 of its rows')
  # the non-zero of A stands at every k position of the first and of the last k-tile, in all three classes' turn
  assert set(range(16)) | set(range(k - 16, k)) <= set(ki.tolist())
  a = np.zeros((m, k), np.float32)
  a[np.arange(m), ki] = av
  w = av.astype(F64)[:, None] * b.astype(F64)[ki]
  want = w.astype(np.float32)
  assert np.array_equal(want.astype(F64), w)            # (one product per element, exact in fp32)
  pads = _pads(k)
  got = _gemm(name, child.padded(a, pads[0]), child.padded(b, pads[1]))
  _explain(got, want, ki)


# ---- 3. dense integer-valued, prepared and not, twice ---------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _dense(name):
  """{offset: (a, b, want)}: tests/test_gemm_split_edges_gpu.py's recipe.  Operands of the longest K; a shorter K takes
  their first K columns / rows, with the second wide pair of the recipe in its own last k-tile.  The products are sums
  of integers below 2^24: exact in fp64 in any order, and in fp32."""
  (m, n), k0 = OUTLINES[name], _k0(name)
  kmax = k0 + max(OFFSETS)
  rng = np.random.RandomState(20261102)
  a_all = rng.randint(-3, 4, size=(m, kmax)).astype(np.float32)
  b_all = rng.randint(-3, 4, size=(kmax, n)).astype(np.float32)
  a_all[:, 5] = rng.randint(-(1 << 18), 1 << 18, size=m)
  b_all[7, :] = rng.randint(-255, 256, size=n)
  head = a_all[:, :k0 - 2].astype(F64).dot(b_all[:k0 - 2].astype(F64))      # shared by the three K
  out = {}
  for off in OFFSETS:
    k = k0 + off
    a, b = a_all[:, :k].copy(), b_all[:k].copy()
    a[:, k - 1] = rng.randint(-(1 << 18), 1 << 18, size=m)
    b[k - 2, :] = rng.randint(-255, 256, size=n)
    prod = head + a[:, k0 - 2:].astype(F64).dot(b[k0 - 2:].astype(F64))
    assert np.abs(prod).max() < 2 ** 24
    out[off] = (a, b, prod.astype(np.float32))
    for x in out[off]:
      x.setflags(write=False)
  return out


@pytest.mark.parametrize('prepared', [False, True])
@pytest.mark.parametrize('off', OFFSETS)
@pytest.mark.parametrize('name', list(OUTLINES))
def test_dense_integer_valued_twice_bit_equal(name, off, prepared):
  from spartan_amd import kernels
  a, b, want = _dense(name)[off]
  pads = _pads(a.shape[1])
  da, db = child.padded(a, pads[0]), child.padded(b, pads[1])
  images = (kernels.gemm_prepare(da, 0), kernels.gemm_prepare(db, 1)) if prepared else None
  first = _gemm(name, da, db, prepared=images)
  second = _gemm(name, da, db, prepared=images)
  assert np.array_equal(_bits(first), _bits(second))
  _explain(first, want)
