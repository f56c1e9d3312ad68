"""The cut of the fp32 GEMM's split tier (spartan_amd/csrc/gemm_split.hpp), checked on the host: v = hi + mid + lo with
three bf16 pieces (round-to-nearest-even on the bit pattern) loses nothing, and the six products the kernel takes
(hh, hm, mh, mm, hl, lh), summed in fp64, differ from the exact product by no more than the header's left-out-terms
bound, 2.004 u sum|a b| (u = 2^-24).  No GPU: this pins the derivation, tests/test_gemm_split_gpu.py the kernels."""
import numpy as np
import pytest

U = 2.0 ** -24
WIN_LO, WIN_HI = 2.0 ** -40, 2.0 ** 40          # the window of gemm_split.hpp: 2^-40 <= |v| < 2^40


def bf16(v):
  """Round-to-nearest-even fp32 -> bf16 (returned as fp32)."""
  b = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
  r = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
  return r.astype(np.uint32).view(np.float32)


def cut(v):
  v = np.asarray(v, np.float32)
  hi = bf16(v)
  r1 = v - hi
  mid = bf16(r1)
  r2 = r1 - mid
  lo = bf16(r2)
  return hi, mid, lo, r1, r2


def _cases():
  rng = np.random.RandomState(20150708)
  n = 200000
  edge = np.array([WIN_LO, np.nextafter(np.float32(WIN_LO), np.float32(1)), np.nextafter(np.float32(WIN_HI), np.float32(0)),
                   WIN_HI / 2, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(2), np.float32(1)),
                   0.0, -0.0], np.float32)
  mant = (1.0 + rng.randint(0, 1 << 23, size=n) * 2.0 ** -23)
  return {
      'uniform': (rng.rand(n) * 2 - 1).astype(np.float32),
      'normal_spread': (rng.randn(n) * 2.0 ** rng.randint(-40, 40, size=n)).astype(np.float32),
      'integers': np.concatenate([rng.randint(-(1 << 24), (1 << 24) + 1, size=n), [1 << 24, -(1 << 24), (1 << 24) - 1, 65535, 65537, 255, 257]]).astype(np.float32),
      'window_edges': np.concatenate([edge, -edge, (mant[:4096] * WIN_LO).astype(np.float32),
                                      (mant[:4096] * (WIN_HI / 2)).astype(np.float32)]),
      'all_ones_mantissa': (np.float32(2) - np.float32(2.0 ** -23)) * (2.0 ** np.arange(-40, 39)).astype(np.float32),
  }


@pytest.mark.parametrize('case', sorted(_cases()))
def test_three_pieces_are_the_value(case):
  v = _cases()[case]
  v = v[(v == 0) | ((np.abs(v) >= WIN_LO) & (np.abs(v) < WIN_HI))]
  assert v.size
  hi, mid, lo, r1, r2 = cut(v)
  v64 = v.astype(np.float64)
  assert np.array_equal(r1.astype(np.float64), v64 - hi.astype(np.float64))                  # v - hi is exact
  assert np.array_equal(r2.astype(np.float64), r1.astype(np.float64) - mid.astype(np.float64))   # (v - hi) - mid too
  assert np.array_equal(lo, r2)                                                              # lo is representable
  assert np.array_equal(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64), v64)
  # no nonzero piece is a bf16 subnormal (bf16 has fp32's exponents): a piece is a multiple of ulp(v) >= 2^-63
  for piece in (hi, mid, lo):
    nz = piece[piece != 0]
    assert nz.size == 0 or np.abs(nz).min() >= 2.0 ** -63
  assert np.all(np.abs(r1) <= 2.0 ** -8 * np.abs(v)) and np.all(np.abs(r2) <= 2.0 ** -16 * np.abs(v))


@pytest.mark.parametrize('case', ['uniform', 'normal_spread', 'integers'])
def test_six_products_within_the_left_out_bound(case):
  rng = np.random.RandomState(7)
  K, rows = 8192, 12
  pool = _cases()[case]
  if case == 'normal_spread':
    pool = pool[(np.abs(pool) >= 2.0 ** -20) & (np.abs(pool) < 2.0 ** 20)]     # (keeps fp64 sums of products exact enough)
  a = pool[rng.randint(0, pool.size, size=(rows, K))]
  b = pool[rng.randint(0, pool.size, size=(rows, K))]
  ah, am, al = [x.astype(np.float64) for x in cut(a)[:3]]
  bh, bm, bl = [x.astype(np.float64) for x in cut(b)[:3]]
  # every product the kernel takes is exact in fp32
  for x, y in ((ah, bh), (ah, bm), (am, bh), (am, bm), (ah, bl), (al, bh)):
    p = x * y
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
  six = ah * bh + ah * bm + am * bh + am * bm + ah * bl + al * bh                # per k: sums of 6 fp64 terms
  exact = a.astype(np.float64) * b.astype(np.float64)
  left = np.abs(am * bl + al * bm + al * bl)
  assert np.all(left <= 2.004 * U * np.abs(exact))
  S = np.abs(exact).sum(axis=1)
  # summed over k, with the fp64 summation's own rounding (K additions of terms <= S) allowed for
  err = np.abs(six.sum(axis=1) - exact.sum(axis=1))
  assert np.all(err <= 2.004 * U * S + 2 * K * 2.0 ** -53 * S), (err / (U * S)).max()


def test_left_out_terms_vanish_when_the_product_is_exact():
  """a with p significant bits, b with q, p + q <= 24: the three products the kernel leaves out are zero, so an
  integer-valued GEMM that is exact in fp32 is exact in the split tier."""
  rng = np.random.RandomState(11)
  for p in range(1, 24):
    q = 24 - p
    a = rng.randint(1 << (p - 1), 1 << p, size=4096).astype(np.float32) * np.float32(2.0) ** rng.randint(-8, 8, size=4096)
    b = rng.randint(1 << (q - 1), 1 << q, size=4096).astype(np.float32)
    _, am, al = [x.astype(np.float64) for x in cut(a)[:3]]
    _, bm, bl = [x.astype(np.float64) for x in cut(b)[:3]]
    assert not np.any(am * bl) and not np.any(al * bm) and not np.any(al * bl)
