"""Times backend.knn (sp_knn: distance and top-k in one pass) with HIP events on the library's stream, and at one size
the NearestNeighbors driver's 'brute' phrasing (all distances to HBM, two full sorts) beside its fused 'auto' path.

  python tools/bench_knn.py [--nq 1024,16384] [--np 262144] [--d 16,64,256] [--k 5,32,128] [--reps 5]
                            [--brute 4096x65536x64x16] [--out profiles/knn_rates.json]

Inputs are standard normal, filled on the device.  The points are rotated through several copies, 512 MiB in all (32
copies at most), so that no call finds its operand in the 256 MiB cache from the call before.  Every figure is the
median of `reps` runs after one warm-up run per copy; one JSON line per case:
  ms              one backend.knn call (events around it; the workspace and the outputs are allocated outside)
  tflops          3 nq np d / ms: one subtract, one multiply, one add per feature and pair
  of_fp32_peak    tflops / 157.3 (the vector fp32 peak counts a fused multiply-add as two; the difference form has no
                  fused operation, so 0.5 is the most this column can reach)
  ms_k1, selection_share   the same call at k = 1, where selection is one compare, and 1 - ms_k1 / ms
The --brute case runs the driver on one worker and times whole kneighbors calls on the host clock (they end with the
result on the host): 'brute', 'auto', and their ratio, next to the kernel's own time at that size, and the share of
the nq x k indices on which the two agree (on real-valued float32 data the 'brute' sum over the features is the
reduction kernel's tree, not the fused kernel's running sum: neighbours closer than their rounding may swap)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import spartan_amd as sp  # noqa: E402
from spartan_amd import devarray as D, kernels  # noqa: E402

PEAK_FP32_VECTOR_TFLOPS = 157.3


def _normal(be, shape, dtype, seed):
  t = be.empty(shape, dtype)
  kernels.random_fill(t, 'normal', seed, 0)
  return t


def _time_knn(be, q, copies, k, reps):
  nq = q.shape[0]
  dist2, idx = be.empty((nq, k), q.dtype), be.empty((nq, k), np.int64)
  for x in copies:
    kernels.knn(q, x, k, dist2, idx)
  D.synchronize()
  out = []
  for r in range(reps):
    x = copies[r % len(copies)]
    e0, e1 = kernels.Event(), kernels.Event()
    e0.record()
    kernels.knn(q, x, k, dist2, idx)
    e1.record()
    e1.synchronize()
    out.append(e0.elapsed_ms(e1))
  return float(np.median(out)), float(min(out)), float(max(out))


def _wall(fn, reps):
  fn()
  out = []
  for _ in range(reps):
    t = time.perf_counter()
    fn()
    out.append((time.perf_counter() - t) * 1e3)
  return float(np.median(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--nq', default='1024,16384')
  ap.add_argument('--np', dest='npts', default='262144')
  ap.add_argument('--d', default='16,64,256')
  ap.add_argument('--k', default='5,32,128')
  ap.add_argument('--dtype', default='float32')
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--brute', default='4096x65536x64x16')
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  dtype = np.dtype(args.dtype)
  rows = []

  def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)
    if args.out:
      with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)

  be = sp.initialize('hip', num_workers=1).backend
  for npts in (int(v) for v in args.npts.split(',') if v):
    for d in (int(v) for v in args.d.split(',') if v):
      n_copies = max(1, min(32, -(-(512 << 20) // (npts * d * dtype.itemsize))))
      copies = [_normal(be, (npts, d), dtype, 100 + c) for c in range(n_copies)]
      for nq in (int(v) for v in args.nq.split(',') if v):
        q = _normal(be, (nq, d), dtype, 7)
        ms_k1, _, _ = _time_knn(be, q, copies, 1, args.reps)
        for k in (int(v) for v in args.k.split(',') if v):
          ms, lo, hi = _time_knn(be, q, copies, k, args.reps)
          tflops = 3.0 * nq * npts * d / ms / 1e9
          emit(dict(kernel='knn', dtype=dtype.name, nq=nq, np=npts, d=d, k=k, ms=round(ms, 4), ms_min=round(lo, 4),
                    ms_max=round(hi, 4), tflops=round(tflops, 3),
                    of_fp32_peak=round(tflops / PEAK_FP32_VECTOR_TFLOPS, 4), ms_k1=round(ms_k1, 4),
                    selection_share=round(1.0 - ms_k1 / ms, 4), copies_of_x=n_copies))
        del q
      del copies
  sp.shutdown()
  if args.brute:
    from spartan_amd.examples.sklearn.neighbors import NearestNeighbors
    nq, npts, d, k = (int(v) for v in args.brute.split('x'))
    rng = np.random.RandomState(20150708)
    qh, xh = rng.randn(nq, d).astype(dtype), rng.randn(npts, d).astype(dtype)
    be = sp.initialize('hip', num_workers=1).backend
    qa, xa = sp.from_numpy(qh).evaluate(), sp.from_numpy(xh).evaluate()
    res = {}

    def run(algorithm):
      res[algorithm] = NearestNeighbors(k, algorithm).fit(xa).kneighbors(qa)

    auto_ms = _wall(lambda: run('auto'), args.reps)
    # the first rows of what was timed, against the oracle and the derived bound of the test-suite
    from tests import knn_cases
    rows_checked = min(8, nq)
    knn_cases.check_real(res['auto'][0][:rows_checked].astype(np.float64) ** 2, res['auto'][1][:rows_checked],
                         qh[:rows_checked], xh, k, d2_dtype=dtype, label='bench auto')
    kernel_ms, _, _ = _time_knn(be, be.from_numpy(qh), [be.from_numpy(xh)], k, args.reps)
    emit(dict(kernel='kneighbors_auto', dtype=dtype.name, nq=nq, np=npts, d=d, k=k, wall_ms=round(auto_ms, 3),
              knn_kernel_ms=round(kernel_ms, 4), rows_checked_against_oracle=rows_checked))
    brute_ms = _wall(lambda: run('brute'), max(1, args.reps // 2))
    same = float(np.mean(res['auto'][1] == res['brute'][1]))
    emit(dict(kernel='kneighbors_brute', dtype=dtype.name, nq=nq, np=npts, d=d, k=k, wall_ms=round(brute_ms, 3),
              ratio_to_auto=round(brute_ms / auto_ms, 2), ratio_to_knn_kernel=round(brute_ms / kernel_ms, 1),
              share_of_indices_equal_to_auto=round(same, 6)))
    sp.shutdown()


if __name__ == '__main__':
  main()
