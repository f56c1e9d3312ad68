"""The k-loop of the split tier's mainloop (sp_gemm_glds_kernel_bf16x3, spartan_amd/csrc/gemm_split.hpp) reads the
fragments of k-tile t + 1 into registers under the MFMAs of k-tile t, two k-tiles per trip with the roles of the two
register buffers swapped, and ends in tails without loads and without reads.  What can go wrong there is a fragment
taken from the wrong LDS stage, from a stage whose tile has not landed or is already being overwritten, or from the wrong
buffer after an odd number of k-tiles.  So, at E1's outline (M, N) = (7681, 8196) of tests/test_gemm_split_edges_gpu.py
and the SHORTEST loops the plan lets through -- K0 is the smallest multiple of 16 the tier takes there, found by asking
the plan --:

  1. dense integer-valued operands (that file's recipe; the fp32 result is exact, so the expected value is the fp64
     product) at K0, K0 + 16 and K0 + 21: both parities of the k-tile count and a K tail, with and without accumulate,
     C filled with NaN where it does not accumulate;
  2. A with one non-zero power of two per row at k = i % K and B dense integers of up to 20 bits, at K0 and K0 + 16:
     every element of C is one exact product from a known k-tile, and a fragment of another k-tile is another row of B;
  3. the products of 1. through images cut beforehand (kernels.gemm_prepare, both operands);
  4. one call of 1. three times into fresh NaN-filled buffers.

Every comparison is bit equality: there is no tolerance.  Integer data has the same bits on the fp32 tier, so each case
asserts first that the plan takes the split tier (sp_gemm_split_workspace_bytes is non-zero) and afterwards that the
library launched its cut kernels: two per call that cuts for itself, none when both operands come cut."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from spartan_amd import _hip  # noqa: E402
from tests import gemm_split_child as child  # noqa: E402

M, N = 7681, 8196
OFFSETS = (0, 16, 21)            # K - K0: even and odd k-tile counts, then K % 16 = 5 and K % 4 = 1 on the odd one
F64 = np.float64


def _ws_bytes(k):
  return _hip.lib().sp_gemm_split_workspace_bytes(_hip.SP_F32, M, N, k)


@functools.lru_cache(maxsize=1)
def _k0():
  """The smallest multiple of 16 at which the plan takes the split tier for (M, N)."""
  for k in range(16, 1 << 16, 16):
    if _ws_bytes(k) != 0:
      print('K0 = %d (%d k-tiles)' % (k, k // 16))
      return k
  raise AssertionError('the plan never takes the split tier at %d x %d' % (M, N))


def _pads(k):
  """Paddings of lda, ldb, ldc: lda and ldb multiples of 4 (the tier's precondition), all three non-zero."""
  return ((-k) % 4 + 4, 4, 12)


def _bits(x):
  return np.ascontiguousarray(x).view(np.uint32)


def _differ(got, want):
  return int(np.count_nonzero(_bits(got) != _bits(want)))


def _cut_launches():
  return _hip.lib().sp_gemm_cut_launches()


def _gemm(a, b, c0, accumulate, prepared=False):
  """c0 (+)= a . b on the split tier.  Unprepared, the call must launch two cut kernels; with both operands cut
  beforehand, none."""
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  k = a.shape[1]
  assert _ws_bytes(k) != 0, k
  pads = _pads(k)
  da, db, c = child.padded(a, pads[0]), child.padded(b, pads[1]), child.padded(c0, pads[2])
  kw = {'prepared_a': kernels.gemm_prepare(da, 0), 'prepared_b': kernels.gemm_prepare(db, 1)} if prepared else {}
  before = _cut_launches()
  kernels.gemm_f32(da, db, c, accumulate=bool(accumulate), **kw)
  assert _cut_launches() - before == (0 if prepared else 2)
  D.synchronize()
  return c.numpy()


@functools.lru_cache(maxsize=1)
def _sentinel():
  c = np.full((M, N), np.nan, np.float32)
  c.setflags(write=False)
  return c


@functools.lru_cache(maxsize=1)
def _dense():
  """{offset: (a, b, want, want_acc)} and c0.  Operands of the longest K; a shorter K takes their first K columns /
  rows, with the wide pairs of the recipe (a wide column of A against small B, a wide row of B against small A) in the
  first k-tile and in its own last one.  The products are sums of integers below 2^24: exact in fp64 in any order."""
  k0 = _k0()
  kmax = k0 + max(OFFSETS)
  rng = np.random.RandomState(20261020)
  a_all = rng.randint(-3, 4, size=(M, kmax)).astype(np.float32)
  b_all = rng.randint(-3, 4, size=(kmax, N)).astype(np.float32)
  a_all[:, 5] = rng.randint(-(1 << 18), 1 << 18, size=M)
  b_all[7, :] = rng.randint(-255, 256, size=N)
  c0 = rng.randint(-9, 10, size=(M, N)).astype(np.float32)
  c0.setflags(write=False)
  head = a_all[:, :k0 - 2].astype(F64).dot(b_all[:k0 - 2].astype(F64))      # shared by the three K
  out = {}
  for off in OFFSETS:
    k = k0 + off
    a, b = a_all[:, :k].copy(), b_all[:k].copy()
    a[:, k - 1] = rng.randint(-(1 << 18), 1 << 18, size=M)
    b[k - 2, :] = rng.randint(-255, 256, size=N)
    prod = head + a[:, k0 - 2:].astype(F64).dot(b[k0 - 2:].astype(F64))
    assert np.abs(prod).max() + 9 < 2 ** 24
    out[off] = (a, b, prod.astype(np.float32), (prod + c0).astype(np.float32))
    for x in out[off]:
      x.setflags(write=False)
  return out, c0


def test_k0_is_the_shortest_loop_the_plan_allows():
  k0 = _k0()
  assert k0 % 16 == 0 and _ws_bytes(k0) != 0
  assert k0 == 16 or _ws_bytes(k0 - 16) == 0
  for off in OFFSETS:
    assert _ws_bytes(k0 + off) != 0, off
  assert (k0 // 16) % 2 != ((k0 + 16) // 16) % 2 and (k0 + 21 + 15) // 16 == k0 // 16 + 2


# ---- 1. dense integer-valued ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('off', OFFSETS)
def test_dense_integer_valued_bit_equal(off, accumulate):
  cases, c0 = _dense()
  a, b, want, want_acc = cases[off]
  got = _gemm(a, b, c0 if accumulate else _sentinel(), accumulate)
  bad = _differ(got, want_acc if accumulate else want)
  print('K = K0 + %d = %d, accumulate=%d: %d elements differ, %d NaN' % (off, a.shape[1], accumulate, bad,
                                                                         np.isnan(got).sum()))
  assert bad == 0


# ---- 2. one product per element, from a known k-tile ------------------------------------------------------------------
@pytest.mark.parametrize('off', OFFSETS[:2])
def test_one_power_of_two_per_row_names_its_k_tile(off):
  k = _k0() + off
  rng = np.random.RandomState(20261021 + off)
  ki = np.arange(M) % k
  av = (2.0 ** rng.randint(-12, 13, size=M) * rng.choice([-1, 1], size=M)).astype(np.float32)
  a = np.zeros((M, k), np.float32)
  a[np.arange(M), ki] = av
  b = rng.randint(-(1 << 20) + 1, 1 << 20, size=(k, N)).astype(np.float32)      # (20 bits: exact in fp32)
  b[b == 0] = 1                                         # (a zero times a negative is -0, and a sum of products is +0)
  want = av[:, None] * b[ki]                            # (a power of two times 20 bits: exact)
  got = _gemm(a, b, _sentinel(), False)
  bad = _bits(got) != _bits(want)
  print('K = %d: %d elements differ, in %d rows' % (k, bad.sum(), bad.any(axis=1).sum()))
  if bad.any():
    rows = np.flatnonzero(bad.any(axis=1))
    raise AssertionError('%d elements in %d rows differ; first rows %s, their k-tiles %s' % (
        bad.sum(), rows.size, rows[:8], ki[rows[:8]] // 16))


# ---- 3. the same products through images cut beforehand ----------------------------------------------------------------
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('off', OFFSETS)
def test_prepared_images_give_the_same_bits(off, accumulate):
  cases, c0 = _dense()
  a, b, want, want_acc = cases[off]
  start = c0 if accumulate else _sentinel()
  unprepared = _gemm(a, b, start, accumulate)
  got = _gemm(a, b, start, accumulate, prepared=True)
  assert _differ(got, unprepared) == 0
  assert _differ(got, want_acc if accumulate else want) == 0


# ---- 4. the same call three times ---------------------------------------------------------------------------------------
def test_three_runs_into_fresh_buffers_are_bit_equal():
  cases, _ = _dense()
  a, b, want, _ = cases[OFFSETS[2]]
  runs = [_gemm(a, b, _sentinel(), False) for _ in range(3)]
  assert _differ(runs[1], runs[0]) == 0 and _differ(runs[2], runs[0]) == 0
  assert _differ(runs[0], want) == 0
