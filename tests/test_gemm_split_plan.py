"""Which shapes the fp32 GEMM's split tier (spartan_amd/csrc/gemm_split.hpp) takes, asked of the library's host-side
workspace queries: no device call, so this runs without a GPU.  The GPU tests of the tier
(tests/test_gemm_split_gpu.py, tests/test_gemm_split_edges_gpu.py) assert that their shapes select it before they
compare anything; this pins the same answers in the CPU suite, so a refit of the cost model that un-selects them is
seen where no GPU runs."""
import os
import subprocess
import sys

import pytest

from spartan_amd import _hip
from tests import test_gemm_split_edges_gpu as edges
from tests import test_gemm_split_gpu as headline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_SHAPES = dict(edges.SHAPES, headline=(headline.M, headline.N, headline.K))


def _split_ws(m, n, k, dtype=_hip.SP_F32):
  return _hip.lib().sp_gemm_split_workspace_bytes(dtype, m, n, k)


@pytest.mark.parametrize('name', sorted(GPU_SHAPES))
def test_gpu_test_shapes_select_the_tier(name):
  m, n, k = GPU_SHAPES[name]
  # the flag's head and three bf16 images of 32 bytes per row and k-tile for each operand
  assert _split_ws(m, n, k) == 512 + (k + 15) // 16 * 3 * 32 * (m + n)
  assert edges._selected(m, n, k) and headline._selected(m, n, k)
  # the tier is only taken where neither split-K nor the balanced kernel is
  assert _hip.lib().sp_gemm_workspace_bytes(_hip.SP_F32, m, n, k) == 0


def test_benchmark_headline_selects_the_tier():
  assert _split_ws(8192, 8192, 8192) == 512 + 512 * 3 * 32 * 16384
  assert _hip.lib().sp_gemm_workspace_bytes(_hip.SP_F32, 8192, 8192, 8192) == 0


@pytest.mark.parametrize('why,dtype,m,n,k', [
    ('fp64', _hip.SP_F64, 8000, 8188, 1000),
    ('N % 4 != 0', _hip.SP_F32, 8000, 8186, 1000),
    ('K = 15', _hip.SP_F32, 8000, 8188, 15),
    ('M = 0', _hip.SP_F32, 0, 8188, 1000),
    ('M < 0', _hip.SP_F32, -8000, 8188, 1000),
    ('N = 0', _hip.SP_F32, 8000, 0, 1000),
    ('N < 0', _hip.SP_F32, 8000, -8188, 1000),
    ('512^3: the tiles do not fill the chip', _hip.SP_F32, 512, 512, 512),
    ('32768^3: images over the 2 GiB cap', _hip.SP_F32, 32768, 32768, 32768),
])
def test_not_taken(why, dtype, m, n, k):
  assert _split_ws(m, n, k, dtype) == 0, why


def test_environment_keeps_the_fp32_tier():
  """SP_GEMM_SPLIT is read once per process: a child"""
  m, n, k = GPU_SHAPES['headline']
  assert _split_ws(m, n, k) > 0
  code = ('from spartan_amd import _hip; '
          'print(_hip.lib().sp_gemm_split_workspace_bytes(_hip.SP_F32, %d, %d, %d))' % (m, n, k))
  out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, SP_GEMM_SPLIT='0'), cwd=ROOT, check=True,
                       stdout=subprocess.PIPE, timeout=300)
  assert int(out.stdout.decode().split()[-1]) == 0
