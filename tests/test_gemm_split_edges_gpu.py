"""The split tier of the fp32 GEMM (spartan_amd/csrc/gemm_split.hpp) through kernels.gemm_f32, term by term and at its
edges, at the smallest shapes that select it (it needs 512 tiles of 256 x 128 and a K of about 500):

  * each of the six piece products (hh, hm, mh, mm, hl, lh) bit-exact at every k position: A with one non-zero per row
    at k = i % K, so that C[i, :] = A[i, k] B[k, :] is ONE product per element, its operands built so that the named
    products are non-zero and the result is exact in fp32 -- a dropped term, or a mid / lo image whose k order differs
    from the hi image's, changes bits;
  * dense integer-valued operands bit-equal to NumPy at shapes that take the row guard and the scalar tail of the cut
    passes, every K % 4, an odd and an even number of k-tiles, a short last group of the tile walk, a last tile of one
    row and one of four columns;
  * the layouts the dispatcher accepts (C a column window at an odd element offset with an odd pitch; A and B views
    inside buffers whose padding is NaN) and one it must refuse (A not 16-byte aligned);
  * the device flag: clean calls between calls that fall back, in one process on the pooled workspace, and values on
    the inside edges of the window, which must not raise it.

The only bars are bit equality and the project's 2 K eps.  The fp32 tier (SP_GEMM_SPLIT=0, read once per process) runs
in a child, once per distinct input."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from spartan_amd import _hip  # noqa: E402
from tests import gemm_split_child as child  # noqa: E402
from tests.test_gemm_split_cut import WIN_HI, WIN_LO, cut  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float32).eps
# name: M, N, K.  With 256 x 256 tiles and k-tiles of 16:
SHAPES = {
    'E1': (7681, 8196, 501),    # 31 tile rows (odd: the last group of the tile walk is short), the last one of ONE row,
                                # M % 32 = 1; last tile column 4 wide; K % 16 = 5, K % 4 = 1, 32 k-tiles
    'E2': (7969, 8188, 527),    # M % 256 = 33, N % 256 = 252, K % 16 = 15, K % 4 = 3, 33 k-tiles
    'E3': (7681, 8192, 498),    # K % 4 = 2
    'E4': (7936, 8196, 512),    # no tail in M or K
}
F64 = np.float64


def pads_of(name):
  """Paddings of lda, ldb, ldc: lda and ldb multiples of 4 (the tier's precondition), all three non-zero."""
  _, _, k = SHAPES[name]
  return ((-k) % 4 + 4, 4, 12)


def _selected(m, n, k):
  """The workspace the split tier asks for (one slab): the flag's head plus three bf16 images per operand."""
  kt = (k + 15) // 16
  return _hip.lib().sp_gemm_split_workspace_bytes(_hip.SP_F32, m, n, k) == 512 + kt * 3 * 32 * (m + n)


def _bits(x):
  return np.ascontiguousarray(x).view(np.uint32)


def _frozen(*arrays):
  for x in arrays:
    x.setflags(write=False)
  return arrays


def _fp32_tier(a, b, c0, pads, accumulate, tmp, tag, offsets=(0, 0, 0), fill=0.0):
  src, dst = os.path.join(tmp, '%s_in.npz' % tag), os.path.join(tmp, '%s_out.npy' % tag)
  np.savez(src, a=a, b=b, c0=c0, pads=np.array(pads), accumulate=np.array(int(accumulate)), offsets=np.array(offsets),
           fill=np.float32(fill))
  env = dict(os.environ, SP_GEMM_SPLIT='0')
  subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'gemm_split_child.py'), src, dst], env=env, cwd=ROOT,
                 check=True, timeout=600)
  out = np.load(dst)
  os.remove(src)
  os.remove(dst)
  return out


def test_shapes_select_the_split_tier():
  for m, n, k in SHAPES.values():
    assert _selected(m, n, k), (m, n, k)


# ---- 1. six terms, bit-exact, at every k position ---------------------------------------------------------------------
# class k % 3 of a k position: significant bits of the planted A values and of row k of B, and the piece products
# that must then be non-zero (an odd p-bit integer has a non-zero mid piece if p > 8, and a lo piece if its first
# remainder has more than 8 significant bits)
A_BITS, B_BITS = (12, 4, 20), (12, 20, 4)
NAMED = (('hh', 'hm', 'mh', 'mm'), ('hh', 'hm', 'hl'), ('hh', 'mh', 'lh'))
SIX = ('hh', 'hm', 'mh', 'mm', 'hl', 'lh')           # what the kernel takes


def _odd_ints(rng, p, size):
  """Random p-bit integers with the top and the bottom bit set, of random sign."""
  v = (1 << (p - 1)) | 1 | (rng.randint(0, 1 << (p - 1), size=size) & ~1)
  return (v * rng.choice([-1, 1], size=size)).astype(F64)


def _scales(rng, p, size):
  """Powers of two that keep a p-bit integer inside the window, 2^-40 <= |v| < 2^40; a quarter each at either end."""
  lo, hi = -40 - (p - 1), 40 - p
  s = rng.randint(lo, hi + 1, size=size)
  end = rng.randint(0, 4, size=size)
  s[end == 0] = lo
  s[end == 1] = hi
  return s


def _draw(seed, m, n, k):
  """planted A values (one per row, at k = i % K), B, and the exponent of each row's product unit"""
  rng = np.random.RandomState(seed)
  ki = np.arange(m) % k
  av, ae = np.empty(m, F64), np.empty(m, np.int64)
  b, be = np.empty((k, n), F64), np.empty(k, np.int64)
  for c in range(3):
    rows = np.flatnonzero(ki % 3 == c)
    ae[rows] = _scales(rng, A_BITS[c], rows.size)
    av[rows] = _odd_ints(rng, A_BITS[c], rows.size) * 2.0 ** ae[rows]
    ks = np.arange(c, k, 3)
    be[ks] = _scales(rng, B_BITS[c], ks.size)
    b[ks] = _odd_ints(rng, B_BITS[c], (ks.size, n)) * (2.0 ** be[ks])[:, None]
  av32, b32 = av.astype(np.float32), b.astype(np.float32)
  assert np.array_equal(av32.astype(F64), av) and np.array_equal(b32.astype(F64), b)
  return ki, av32, b32, ae + be[ki]


def _terms_bite(ki, av, b):
  """The condition without which the test could pass with a piece that is zero: for each class, leaving any one of its
  named products out of the six changes the fp32 result in at least 3/4 of the class's rows (seen on every eighth
  column and the last four: a lower bound).  Also: the six products are the whole product."""
  n = b.shape[1]
  cols = np.unique(np.r_[0:n:8, n - 4:n])
  for c in range(3):
    rows = np.flatnonzero(ki % 3 == c)
    pa = dict(zip('hml', [x.astype(F64)[:, None] for x in cut(av[rows])[:3]]))
    bsub = b[np.ix_(ki[rows], cols)]
    pb = dict(zip('hml', [x.astype(F64) for x in cut(bsub)[:3]]))
    six = {t: pa[t[0]] * pb[t[1]] for t in SIX}
    total = sum(six.values())                            # (multiples of one unit per row, below 2^26 of it: exact in fp64)
    exact = av[rows].astype(F64)[:, None] * bsub.astype(F64)
    assert np.array_equal(total, exact)
    want = exact.astype(np.float32)
    for t in NAMED[c]:
      changed = ((total - six[t]).astype(np.float32) != want).any(axis=1).mean()
      if changed < 0.75:
        return False
  return True


@functools.lru_cache(maxsize=1)
def _six_term_case(name):
  m, n, k = SHAPES[name]
  for seed in range(20150708, 20150716):
    ki, av, b, ue = _draw(seed, m, n, k)
    if _terms_bite(ki, av, b):
      break
  else:
    raise AssertionError('no draw in which every named piece product is non-zero in 3/4 of its rows')
  for v in (av, b):
    assert np.all((np.abs(v) >= WIN_LO) & (np.abs(v) < WIN_HI))               # inside the window ...
    assert np.abs(v).min() < 2 * WIN_LO and np.abs(v).max() >= WIN_HI / 2     # ... and at both of its ends
  a = np.zeros((m, k), np.float32)
  a[np.arange(m), ki] = av
  # C[i, :] = A[i, k_i] B[k_i, :] by gather in fp64, exactly representable in fp32; c0: small multiples of the row's
  # product unit, kept only where product + c0 is exact in fp32 too
  rng = np.random.RandomState(9)
  b64 = b.astype(F64)
  want = np.empty((m, n), np.float32)
  c0 = np.empty((m, n), np.float32)
  want_acc = np.empty((m, n), np.float32)
  for r0 in range(0, m, 1024):
    r = slice(r0, min(r0 + 1024, m))
    w = av[r].astype(F64)[:, None] * b64[ki[r]]
    want[r] = w
    assert np.array_equal(want[r].astype(F64), w)
    c = rng.randint(-8, 9, size=w.shape) * (2.0 ** ue[r])[:, None]      # (at most 4 bits: representable)
    s = w + c                                                           # (exact: below 2^25 of the unit)
    want_acc[r] = s
    keep = want_acc[r].astype(F64) == s
    c0[r] = np.where(keep, c, 0)
    want_acc[r] = np.where(keep, s, w)
  assert np.count_nonzero(c0) > 0.8 * c0.size
  return _frozen(a, b, c0, want, want_acc)


@pytest.mark.parametrize('name,accumulate', [('E1', False), ('E1', True), ('E2', False), ('E2', True)])
def test_six_piece_products_bit_exact_at_every_k(name, accumulate):
  m, n, k = SHAPES[name]
  assert _selected(m, n, k)
  a, b, c0, want, want_acc = _six_term_case(name)
  got = child.run(a, b, c0, pads_of(name), accumulate)
  bad = _bits(got) != _bits(want_acc if accumulate else want)
  print('%s accumulate=%d: %d elements differ, in %d rows' % (name, accumulate, bad.sum(), bad.any(axis=1).sum()))
  if bad.any():
    rows = np.flatnonzero(bad.any(axis=1))
    raise AssertionError('%d elements in %d rows differ; first rows %s, their k %s, k %% 3 of all bad rows %s' % (
        bad.sum(), rows.size, rows[:8], rows[:8] % k, np.unique((rows % k) % 3)))


# ---- 2. dense integer-valued ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _dense_case(name):
  """tests/test_gemm_split_gpu.py's recipe (small integers, one wide column of A against small B, one wide row of B
  against small A) with a second wide pair in the last k-tile"""
  m, n, k = SHAPES[name]
  rng = np.random.RandomState(3)
  a = rng.randint(-3, 4, size=(m, k)).astype(np.float32)
  b = rng.randint(-3, 4, size=(k, n)).astype(np.float32)
  a[:, 5] = rng.randint(-(1 << 18), 1 << 18, size=m)
  b[7, :] = rng.randint(-255, 256, size=n)
  a[:, k - 1] = rng.randint(-(1 << 18), 1 << 18, size=m)
  b[k - 2, :] = rng.randint(-255, 256, size=n)
  c0 = rng.randint(-9, 10, size=(m, n)).astype(np.float32)
  prod = a.astype(F64).dot(b.astype(F64))
  assert np.abs(prod).max() + 9 < 2 ** 24
  return _frozen(a, b, c0, prod.astype(np.float32), (prod + c0).astype(np.float32))


@pytest.mark.parametrize('name,accumulate', [(s, acc) for s in ('E2', 'E3', 'E4', 'E1') for acc in (False, True)])
def test_dense_integer_valued_bit_equal(name, accumulate):
  m, n, k = SHAPES[name]
  assert _selected(m, n, k)
  a, b, c0, want, want_acc = _dense_case(name)
  got = child.run(a, b, c0, pads_of(name), accumulate)
  np.testing.assert_array_equal(got, want_acc if accumulate else want)


# ---- 3. layouts (E1) --------------------------------------------------------------------------------------------------
def test_c_window_at_an_odd_offset_and_pitch_keeps_what_surrounds_it():
  m, n, k = SHAPES['E1']
  assert _selected(m, n, k)
  a, b, c0, _, want_acc = _dense_case('E1')
  pads, sentinel = pads_of('E1')[:2] + (3,), np.float32(-1234.5)
  assert (n + pads[2]) % 2 == 1
  got, whole = child.run(a, b, c0, pads, True, offsets=(0, 0, 1), fill=sentinel, whole=True)
  np.testing.assert_array_equal(got, want_acc)
  ld = n + pads[2]
  assert whole.size == 1 + m * ld
  outside = np.ones(whole.size, bool)
  outside[1:].reshape(m, ld)[:, :n] = False
  assert outside.sum() == 1 + m * pads[2]
  assert np.all(_bits(whole)[outside] == _bits(np.array([sentinel]))[0])


@pytest.fixture(scope='module')
def uniform():
  """E1, uniform [-1, 1); column K - 3 of A and row K - 3 of B are zero (what the inside-edge test plants there meets
  zeros).  With the fp64 product."""
  m, n, k = SHAPES['E1']
  rng = np.random.RandomState(4)
  a = (rng.rand(m, k) * 2 - 1).astype(np.float32)
  b = (rng.rand(k, n) * 2 - 1).astype(np.float32)
  a[:, k - 3] = 0
  b[k - 3, :] = 0
  return _frozen(a, b, np.zeros((m, n), np.float32), a.astype(F64).dot(b.astype(F64)))


@pytest.fixture(scope='module')
def uniform_fp32_tier(uniform, tmp_path_factory):
  a, b, c0, _ = uniform
  return _fp32_tier(a, b, c0, pads_of('E1'), False, str(tmp_path_factory.mktemp('fp32_tier')), 'clean')


def test_views_inside_nan_padded_buffers(uniform, uniform_fp32_tier):
  """A, B and C start 4 elements (16 bytes) into buffers that are NaN wherever the views are not: a cut pass that read
  beyond K or N, or in front of a view, would put a NaN into an image or raise the flag -- and then the result would be
  NaN, or the fp32 tier's bits."""
  m, n, k = SHAPES['E1']
  assert _selected(m, n, k)
  a, b, c0, ref = uniform
  got = child.run(a, b, c0, pads_of('E1'), False, offsets=(4, 4, 4), fill=np.float32(np.nan))
  err = np.abs(got - ref).max()
  differ = (_bits(got) != _bits(uniform_fp32_tier)).sum()
  print('E1 NaN padding: max error %.3e (bar 2 K eps = %.3e); %d of %d elements differ from the fp32 tier' % (
      err, 2 * k * EPS, differ, got.size))
  assert err <= 2 * k * EPS
  assert differ > 0


def test_unaligned_a_leaves_the_tier(uniform, tmp_path):
  m, n, k = SHAPES['E1']
  assert _selected(m, n, k)
  a, b, c0, ref = uniform
  got = child.run(a, b, c0, pads_of('E1'), False, offsets=(1, 0, 0))
  want = _fp32_tier(a, b, c0, pads_of('E1'), False, str(tmp_path), 'unaligned', offsets=(1, 0, 0))
  assert np.array_equal(_bits(got), _bits(want))
  assert np.abs(got - ref).max() <= 2 * k * EPS


# ---- 4. the flag (E1, one process) ------------------------------------------------------------------------------------
def test_flag_is_cleared_between_calls_and_not_raised_inside_the_window(uniform, uniform_fp32_tier, tmp_path):
  m, n, k = SHAPES['E1']
  assert _selected(m, n, k)
  a, b, c0, _ = uniform
  pads = pads_of('E1')
  clean = child.run(a, b, c0, pads, False)
  differ = (_bits(clean) != _bits(uniform_fp32_tier)).sum()
  print('E1 clean: %d of %d elements differ from the fp32 tier' % (differ, clean.size))
  assert differ > 0                                   # so bit equality with `clean` below says: the split tier ran

  sub = a.copy()
  sub[m - 1, k - 1] = np.float32(2.0 ** -130)         # K % 4 = 1: the scalar tail lane of the cut, in its guarded last row
  got = child.run(sub, b, c0, pads, False)
  assert np.array_equal(_bits(got), _bits(_fp32_tier(sub, b, c0, pads, False, str(tmp_path), 'subnormal')))
  assert np.array_equal(_bits(child.run(a, b, c0, pads, False)), _bits(clean))

  inf = b.copy()
  inf[k - 1, n - 1] = np.inf
  got = child.run(a, inf, c0, pads, False)
  assert np.array_equal(_bits(got), _bits(_fp32_tier(a, inf, c0, pads, False, str(tmp_path), 'inf')))
  assert np.array_equal(_bits(child.run(a, b, c0, pads, False)), _bits(clean))

  # the inside edges of the window against a zero row of B: same bits as with the column zero
  edge = a.copy()
  below_hi = np.nextafter(np.float32(WIN_HI), np.float32(0))
  edge[:, k - 3] = np.resize(np.array([WIN_LO, -WIN_LO, below_hi, -below_hi], np.float32), m)
  assert not np.any(b[k - 3]) and not np.any(a[:, k - 3])
  assert np.array_equal(_bits(child.run(edge, b, c0, pads, False)), _bits(clean))
