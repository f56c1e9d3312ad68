"""Child of tests/test_gemm_split_gpu.py and tests/test_gemm_split_edges_gpu.py: c (+)= a . b through kernels.gemm_f32
in a process of its own, so that the parent can choose SP_GEMM_SPLIT (read once per process) in the environment.
argv: in.npz out.npy; the .npz holds a, b, c0 (the initial c), the paddings of the three leading dimensions and
`accumulate`, and optionally `offsets` (the element offsets of the a, b and c views inside their padded buffers) and
`fill` (what the buffers hold outside the views: in front of them, behind every row and behind the last one).  Without
the two the views start their buffers and the padding is zeros."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)


def placed(arr, pad, offset=0, fill=0):
  """(buffer, view): `arr` as a device view with row pitch cols + pad that starts `offset` elements into a 1-D device
  buffer of offset + rows * (cols + pad) elements; every element of the buffer outside the view is `fill`."""
  from spartan_amd import devarray as D
  rows, cols = arr.shape
  ld = cols + pad
  host = np.full(offset + rows * ld, fill, arr.dtype)
  host[offset:].reshape(rows, ld)[:, :cols] = arr
  buf = D.from_numpy(host)
  return buf, buf[offset:].reshape(rows, ld)[:, :cols]


def padded(arr, pad):
  return placed(arr, pad)[1]


def run(a, b, c0, pads, accumulate, offsets=(0, 0, 0), fill=0, whole=False):
  """The c view after the GEMM; with `whole`, (the c view, the whole 1-D c buffer)."""
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  cbuf, c = placed(c0, pads[2], offsets[2], fill)
  kernels.gemm_f32(placed(a, pads[0], offsets[0], fill)[1], placed(b, pads[1], offsets[1], fill)[1], c,
                   accumulate=bool(accumulate))
  D.synchronize()
  return (c.numpy(), cbuf.numpy()) if whole else c.numpy()


if __name__ == '__main__':
  z = np.load(sys.argv[1])
  np.save(sys.argv[2], run(z['a'], z['b'], z['c0'], [int(x) for x in z['pads']], int(z['accumulate']),
                           [int(x) for x in z['offsets']] if 'offsets' in z.files else (0, 0, 0),
                           z['fill'][()] if 'fill' in z.files else 0))
