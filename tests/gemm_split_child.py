"""Child of tests/test_gemm_split_gpu.py: c (+)= a . b through kernels.gemm_f32 in a process of its own, so that the
parent can choose SP_GEMM_SPLIT (read once per process) in the environment.  argv: in.npz out.npy; the .npz holds a, b,
c0 (the initial c), the paddings of the three leading dimensions and `accumulate`."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)


def padded(arr, pad):
  from spartan_amd import devarray as D
  return D.from_numpy(np.pad(arr, ((0, 0), (0, pad))))[:, :arr.shape[1]]


def run(a, b, c0, pads, accumulate):
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  c = padded(c0, pads[2])
  kernels.gemm_f32(padded(a, pads[0]), padded(b, pads[1]), c, accumulate=bool(accumulate))
  D.synchronize()
  return c.numpy()


if __name__ == '__main__':
  z = np.load(sys.argv[1])
  np.save(sys.argv[2], run(z['a'], z['b'], z['c0'], [int(x) for x in z['pads']], int(z['accumulate'])))
