"""Plain NumPy restatement of sp_random_fill (csrc/random.hip, include/spartan_hip.h): Philox4x32-10 and the three
output maps.  Pure NumPy; nothing here reads the library.

Block.  Elements 2p and 2p + 1 of the stream of `seed` come from the Philox block of pair p: counter words
(p & 0xffffffff, p >> 32, CTR_HI & 0xffffffff, CTR_HI >> 32), key words (seed & 0xffffffff, seed >> 32), ten rounds
with the multipliers and Weyl key increments of Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC11).
A fill of n elements at an even `offset` starts at pair offset / 2.

Maps.  With x, y, z, w the four output words, ra = x << 32 | y and rb = z << 32 | w:
  uniform   a = (ra >> 11) * 2^-53, b = (rb >> 11) * 2^-53.  float64: as they are.  float32: float32(a), except that a
            result of 1.0 (every a >= 1 - 2^-25 rounds there) is the largest float32 below 1: the range is [0, 1).
  normal    rad = sqrt(-2 log(1 - a)), ang = (2 pi) * b, elements rad cos(ang) and rad sin(ang).  1 - a and the product
            with the double nearest to 2 pi are rounded to double as the kernel rounds them; log, sqrt, cos and sin are
            evaluated in numpy.longdouble.
  randint   lo + ra % (hi - lo) and lo + rb % (hi - lo).
"""
import functools

import numpy as np

CTR_HI = 0x5350415254414e          # "SPARTAN": the constant high counter half of csrc/random.hip
M0, M1 = 0xD2511F53, 0xCD9E8D57     # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85     # the key increments (golden ratio, sqrt(3) - 1)
MASK32 = np.uint64(0xffffffff)
TWO_PI = 6.283185307179586476925    # the literal of the kernel: the double nearest to 2 pi
LD = np.longdouble
BELOW_ONE_F32 = np.nextafter(np.float32(1), np.float32(0))


def philox4x32_10(counter, key):
  """counter [..., 4] and key [..., 2] (anything that converts to uint32 words) -> the output block [..., 4] uint32."""
  c = np.asarray(counter, dtype=np.uint64)
  k = np.asarray(key, dtype=np.uint64)
  c0, c1, c2, c3 = (c[..., i] & MASK32 for i in range(4))
  k0, k1 = k[..., 0] & MASK32, k[..., 1] & MASK32
  for _ in range(10):
    p0 = np.uint64(M0) * c0          # 32 x 32 -> 64 bits: no wrap in uint64
    p1 = np.uint64(M1) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
    k0 = (k0 + np.uint64(W0)) & MASK32
    k1 = (k1 + np.uint64(W1)) & MASK32
  return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def blocks(seed, first_pair, npairs):
  """The output blocks [npairs, 4] of pairs first_pair .. first_pair + npairs - 1 (pair numbers wrap at 2^64)."""
  p = (np.arange(npairs, dtype=np.uint64) + np.uint64(int(first_pair) & (2**64 - 1)))
  ctr = np.empty((npairs, 4), np.uint64)
  ctr[:, 0] = p & MASK32
  ctr[:, 1] = p >> np.uint64(32)
  ctr[:, 2] = CTR_HI & 0xffffffff
  ctr[:, 3] = CTR_HI >> 32
  seed = int(seed) & (2**64 - 1)
  key = np.array([seed & 0xffffffff, seed >> 32], np.uint64)
  return philox4x32_10(ctr, np.broadcast_to(key, (npairs, 2)))


@functools.lru_cache(maxsize=8)
def _halves(seed, offset, n):
  """(ra, rb) uint64 [pairs], read-only, for the n elements at the even stream position `offset`."""
  assert offset % 2 == 0, 'a fill starts at an even stream position'
  b = blocks(seed, offset // 2, (n + 1) // 2).astype(np.uint64)
  ra, rb = (b[:, 0] << np.uint64(32)) | b[:, 1], (b[:, 2] << np.uint64(32)) | b[:, 3]
  ra.setflags(write=False)
  rb.setflags(write=False)
  return ra, rb


def _interleave(a, b, n):
  out = np.empty(2 * len(a), dtype=a.dtype)
  out[0::2], out[1::2] = a, b
  return out[:n]


def uniforms53(seed, offset, n):
  """(a, b) float64 [pairs]: the two 53-bit uniforms of every pair."""
  ra, rb = _halves(seed, offset, n)
  scale = 2.0 ** -53
  return (ra >> np.uint64(11)).astype(np.float64) * scale, (rb >> np.uint64(11)).astype(np.float64) * scale


def to_float32_unit(u):
  """float32(u) for u in [0, 1), with the results that round to 1.0 moved to the largest float32 below 1."""
  f = np.asarray(u, np.float64).astype(np.float32)
  return np.where(f >= np.float32(1), BELOW_ONE_F32, f).astype(np.float32)


def uniform(seed, offset, n, dtype=np.float64):
  a, b = uniforms53(seed, offset, n)
  u = _interleave(a, b, n)
  if np.dtype(dtype) == np.float64:
    return u
  assert np.dtype(dtype) == np.float32
  return to_float32_unit(u)


def randint(seed, offset, n, lo, hi, dtype=np.int64):
  assert hi > lo and hi - lo < 2**64
  ra, rb = _halves(seed, offset, n)
  rng = np.uint64(hi - lo)
  # lo + r % range in two's complement, as the kernel's int64 addition
  vals = (_interleave(ra % rng, rb % rng, n) + np.uint64(int(lo) & (2**64 - 1))).view(np.int64)
  if np.dtype(dtype) == np.int64:
    return vals
  assert np.dtype(dtype) == np.int32 and -2**31 <= lo and hi <= 2**31, 'an int32 fill holds a range inside int32'
  return vals.astype(np.int32)


def normal_from_uniforms(a, b):
  """(first, second, rad) in longdouble from float64 uniforms: the Box-Muller pair and its radius."""
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  x = 1.0 - a                                   # rounded to double, in (0, 1]
  ang = TWO_PI * b                              # rounded to double
  with np.errstate(divide='ignore'):
    rad = np.sqrt(LD(-2) * np.log(x.astype(LD)))
  angl = ang.astype(LD)
  return rad * np.cos(angl), rad * np.sin(angl), rad


def normal(seed, offset, n):
  """(values, rad) longdouble [n]: the normal stream and, per element, the radius of its pair."""
  a, b = uniforms53(seed, offset, n)
  first, second, rad = normal_from_uniforms(a, b)
  return _interleave(first, second, n), _interleave(rad, rad, n)


# OpenCL 3.0 full-profile limits for double precision, in ulp (table 7.4 of the OpenCL C specification): the
# documented accuracy of the device library's log, sqrt, sin, cos
ULP_LOG, ULP_SQRT, ULP_SIN, ULP_COS = 3, 0, 4, 4
# one output takes log, sqrt, one of sin / cos, and two products (-2 * log, rad * cos); 4 x for ulp <= 2^-52 |value|
# = 2 x 2^-53 and a factor 2 of slack on first-order terms.  See tests/test_random.py for the derivation.
NORMAL_K = 4 * (ULP_LOG + ULP_SQRT + max(ULP_SIN, ULP_COS) + 2)
