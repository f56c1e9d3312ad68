"""The split tier of the fp32 GEMM (spartan_amd/csrc/gemm_split.hpp) through kernels.gemm_f32, at a shape that selects
it: partial edge tiles in M and N, a K that is no multiple of the k-tile, padded lda / ldb / ldc, with and without
`accumulate`.  Integer-valued operands bit-equal to NumPy; uniform [-1, 1) within 2 K eps and no worse than the fp32
tier (SP_GEMM_SPLIT=0, read once per process: a child); operands outside the tier's window bit-equal to the fp32
tier, which proves the gated fallback."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from spartan_amd import _hip  # noqa: E402
from tests import gemm_split_child as child  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N, K = 8000, 8188, 1000              # 32 x 64 tiles of 256 x 128 (4 full rounds), last row / column of tiles partial
PADS = (8, 4, 12)                       # lda = 1008, ldb = 8192, ldc = 8200
EPS = np.finfo(np.float32).eps


def _selected(m, n, k):
  """The workspace the split tier asks for (one slab): the flag's head plus three bf16 images per operand."""
  kt = (k + 15) // 16
  return _hip.lib().sp_gemm_split_workspace_bytes(_hip.SP_F32, m, n, k) == 512 + kt * 3 * 32 * (m + n)


def _fp32_tier(a, b, c0, accumulate, tmp_path, tag):
  src, dst = str(tmp_path / ('%s_in.npz' % tag)), str(tmp_path / ('%s_out.npy' % tag))
  np.savez(src, a=a, b=b, c0=c0, pads=np.array(PADS), accumulate=np.array(int(accumulate)))
  env = dict(os.environ, SP_GEMM_SPLIT='0')
  subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'gemm_split_child.py'), src, dst], env=env, cwd=ROOT,
                 check=True, timeout=600)
  return np.load(dst)


def test_shape_selects_the_split_tier():
  assert _selected(M, N, K)
  assert not _selected(512, 512, 512)


@pytest.mark.parametrize('accumulate', [False, True])
def test_integer_valued_bit_equal(accumulate):
  rng = np.random.RandomState(3)
  a = rng.randint(-3, 4, size=(M, K)).astype(np.float32)
  b = rng.randint(-3, 4, size=(K, N)).astype(np.float32)
  a[:, 5] = rng.randint(-(1 << 18), 1 << 18, size=M)           # a few wide ones: all three pieces of an operand at work
  b[7, :] = rng.randint(-255, 256, size=N)
  c0 = rng.randint(-9, 10, size=(M, N)).astype(np.float32)
  assert _selected(M, N, K)
  got = child.run(a, b, c0, PADS, accumulate)
  want = a.astype(np.float64).dot(b.astype(np.float64)) + (c0 if accumulate else 0)
  assert np.abs(want).max() < 2 ** 24
  np.testing.assert_array_equal(got, want.astype(np.float32))


def test_uniform_within_bar_and_no_worse_than_fp32_tier(tmp_path):
  rng = np.random.RandomState(4)
  a = (rng.rand(M, K) * 2 - 1).astype(np.float32)
  b = (rng.rand(K, N) * 2 - 1).astype(np.float32)
  c0 = np.zeros((M, N), np.float32)
  assert _selected(M, N, K)
  got = child.run(a, b, c0, PADS, False)
  ref = a.astype(np.float64).dot(b.astype(np.float64))
  err = np.abs(got - ref).max()
  fp32 = _fp32_tier(a, b, c0, False, tmp_path, 'uniform')
  err32 = np.abs(fp32 - ref).max()
  print('split tier max error %.3e, fp32 tier %.3e, ratio %.3f (bar 2 K eps = %.3e)' % (err, err32, err / err32, 2 * K * EPS))
  assert err <= 2 * K * EPS
  assert err <= err32


@pytest.mark.parametrize('which,accumulate', [('nan_inf_above_below', True), ('above', False), ('below', False)])
def test_outside_the_window_is_the_fp32_tier_bit_for_bit(which, accumulate, tmp_path):
  """uniform data is NOT bit-equal between the tiers (different summation), so equality here is the fallback's doing"""
  rng = np.random.RandomState(5)
  a = (rng.rand(M, K) * 2 - 1).astype(np.float32)
  b = (rng.rand(K, N) * 2 - 1).astype(np.float32)
  c0 = (rng.rand(M, N) * 2 - 1).astype(np.float32)
  if which == 'nan_inf_above_below':
    b[3, 17] = np.nan
    b[900, 8187] = np.inf
    b[512, 4000] = np.float32(2.0 ** 41)
    b[999, 0] = np.float32(2.0 ** -41)
  elif which == 'above':
    a[7999, 999] = np.float32(-2.0 ** 40)         # the window is 2^-40 <= |v| < 2^40
  else:
    a[0, 0] = np.float32(np.nextafter(np.float32(2.0 ** -40), np.float32(0)))
  assert _selected(M, N, K)
  got = child.run(a, b, c0, PADS, accumulate)
  want = _fp32_tier(a, b, c0, accumulate, tmp_path, which)
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
