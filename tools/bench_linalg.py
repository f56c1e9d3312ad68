"""Times sp_potrf and sp_trsm_rlt with HIP events, next to the host route a driver would otherwise take for the same
tile (device-to-host copy, SciPy's LAPACK, copy back) and to the GEMM rate of the same dtype; and sp_syevj (wall
time: the call waits for the device once per sweep) next to its host route (copy, LAPACK's syevd, two copies back).

  python tools/bench_linalg.py [--orders 2048,4096,8192] [--syev 64,256,1024] [--reps 3] [--out profiles/linalg_rates.json]

Every figure is the median of `reps` runs after one warm-up run; prints one JSON line per case."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import spartan_amd as sp  # noqa: E402
from spartan_amd import _hip, devarray as D, kernels  # noqa: E402


def _events(fn, reps):
  fn()
  D.synchronize()
  out = []
  for _ in range(reps):
    e0, e1 = kernels.Event(), kernels.Event()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    out.append(e0.elapsed_ms(e1))
  return float(np.median(out))


def _wall(fn, reps):
  fn()
  out = []
  for _ in range(reps):
    t = time.perf_counter()
    fn()
    out.append((time.perf_counter() - t) * 1e3)
  return float(np.median(out))


def _plain_gemm(a, b, c):
  g = a.shape[0]
  kernels.check(_hip.lib().sp_gemm_ws(_hip.sp_dtype(kernels.np_dtype_of(a)), C.c_void_p(a.data_ptr()), g,
                                      C.c_void_p(b.data_ptr()), g, C.c_void_p(c.data_ptr()), g, g, g, g, 0, None, 0,
                                      kernels._stream()))


def _spd(n, dtype):
  g = np.random.RandomState(20150708).randn(n, n).astype(dtype)
  return (g.dot(g.T) + n * np.eye(n, dtype=dtype)).astype(dtype)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--orders', default='2048,4096,8192')
  ap.add_argument('--dtypes', default='float32,float64')
  ap.add_argument('--reps', type=int, default=3)
  ap.add_argument('--trsm', default='65536x256')
  ap.add_argument('--syev', default='64,256,1024')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  from scipy.linalg import lapack
  be = sp.initialize('hip', num_workers=1).backend
  rows = []
  for name in args.dtypes.split(','):
    dtype = np.dtype(name)
    # the GEMM rate of this dtype on a square product, the yardstick of the 'fraction' column: sp_gemm_ws WITHOUT a
    # workspace, so that fp32 stays on the plain MFMA tier, the one sp_potrf's updates run on (with the workspace
    # kernels.gemm hands it, a product of this size goes to the bf16 split tier)
    g = 4096
    a, b, c = (be.from_numpy(np.ones((g, g), dtype)) for _ in range(3))
    gemm_ms = _events(lambda: _plain_gemm(a, b, c), args.reps)
    gemm_rate = 2.0 * g ** 3 / gemm_ms / 1e9
    del a, b, c
    for n in (int(v) for v in args.orders.split(',') if v):
      host = _spd(n, dtype)
      src = be.from_numpy(host)
      work, info = be.empty((n, n), dtype), be.zeros((1,), np.int32)

      def device():
        be.paste(work, (slice(0, n), slice(0, n)), src)
        kernels.potrf(work, info)

      copy_ms = _events(lambda: be.paste(work, (slice(0, n), slice(0, n)), src), args.reps)
      dev_ms = _events(device, args.reps) - copy_ms
      assert int(info.numpy()[0]) == 0
      potrf = lapack.get_lapack_funcs(('potrf',), (host,))[0]

      def host_route():
        h = src.numpy()
        low, bad = potrf(h, lower=1, clean=1)
        be.from_numpy(low)
        D.synchronize()

      host_ms = _wall(host_route, args.reps)
      lapack_ms = _wall(lambda: potrf(host, lower=1, clean=1), args.reps)
      rate = n ** 3 / 3.0 / dev_ms / 1e9
      rows.append(dict(kernel='potrf', dtype=name, n=n, device_ms=round(dev_ms, 3), tflops=round(rate, 3),
                       fraction_of_gemm=round(rate / gemm_rate, 4), gemm_tflops=round(gemm_rate, 2),
                       host_route_ms=round(host_ms, 3), lapack_only_ms=round(lapack_ms, 3)))
      print(json.dumps(rows[-1]), flush=True)
      del src, work
    if args.trsm:
      m, n = (int(v) for v in args.trsm.split('x'))
      low = np.linalg.cholesky(_spd(n, np.float64)).astype(dtype)
      bh = np.random.RandomState(1).randn(m, n).astype(dtype)
      lt, src, work = be.from_numpy(low), be.from_numpy(bh), be.empty((m, n), dtype)

      def device():
        be.paste(work, (slice(0, m), slice(0, n)), src)
        kernels.trsm_rlt(work, lt)

      copy_ms = _events(lambda: be.paste(work, (slice(0, m), slice(0, n)), src), args.reps)
      dev_ms = _events(device, args.reps) - copy_ms
      trtrs = lapack.get_lapack_funcs(('trtrs',), (low, bh))[0]

      def host_route():
        h = src.numpy()
        x, bad = trtrs(low, h.T, lower=1)
        be.from_numpy(np.ascontiguousarray(x.T))
        D.synchronize()

      host_ms = _wall(host_route, args.reps)
      rate = float(m) * n * n / dev_ms / 1e9
      rows.append(dict(kernel='trsm_rlt', dtype=name, m=m, n=n, device_ms=round(dev_ms, 3), tflops=round(rate, 3),
                       fraction_of_gemm=round(rate / gemm_rate, 4), gemm_tflops=round(gemm_rate, 2),
                       host_route_ms=round(host_ms, 3)))
      print(json.dumps(rows[-1]), flush=True)
    for n in (int(v) for v in args.syev.split(',') if v):
      g = np.random.RandomState(20150708).randn(n, n)
      host = ((g + g.T) / 2).astype(dtype)
      src = be.from_numpy(host)
      w, v, info = be.empty((n,), dtype), be.empty((n, n), dtype), be.zeros((1,), np.int32)
      sweeps = []

      def device():
        sweeps.append(kernels.syevj(src, w, v, info))
        D.synchronize()

      dev_ms = _wall(device, args.reps)
      assert int(info.numpy()[0]) == 0
      syevd = lapack.get_lapack_funcs(('syevd',), (host,))[0]

      def host_route():
        h = src.numpy()
        wh, vh, bad = syevd(h, lower=1)
        be.from_numpy(wh)
        be.from_numpy(np.ascontiguousarray(vh))
        D.synchronize()

      host_ms = _wall(host_route, args.reps)
      lapack_ms = _wall(lambda: syevd(host, lower=1), args.reps)
      rows.append(dict(kernel='syev', dtype=name, n=n, sweeps=sweeps[-1], device_wall_ms=round(dev_ms, 3),
                       host_route_ms=round(host_ms, 3), lapack_only_ms=round(lapack_ms, 3)))
      print(json.dumps(rows[-1]), flush=True)
  sp.shutdown()
  if args.out:
    with open(args.out, 'w') as f:
      json.dump(rows, f, indent=1)


if __name__ == '__main__':
  main()
