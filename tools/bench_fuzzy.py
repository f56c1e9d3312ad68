"""Times one fuzzy k-means step on a row tile (sp_fuzzy_step) with HIP events on the library's stream, 'fused' against
'map2' on the same build in the same run.

  python tools/bench_fuzzy.py [--reps 5] [--out profiles/fuzzy_rates.json]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Steps (m = 2, the driver's default):
  float32   1 250 000 x 256 points, k = 1024: one row tile of BASELINE configs[3]
  float64   200 000 x 64 points, k = 256
Points and centres are drawn on the host from a seed.  Per step the variants are warmed up once each and then timed
ALTERNATELY, `reps` rounds; every figure is the median (min and max beside it).  Variants, as the driver's tile bodies
run them (spartan_amd/examples/fuzzy_kmeans.py):
  fused     backend.fuzzy_step(points, centers, m): labels, sums, wsum; nothing of size n x k exists
  fused_u   the same call with want_u=True: the kernel's second sweep of the centres and the n x k write on top
  map2      what 'map2' does on a tile: U = fuzzy_step(want_u=True)[3], argmax(U, axis=1), W = U ** m,
            dot(W.T, X) (the GEMM) and sum(W, axis=0) -- five kernels' worth of n x k traffic
One JSON line per variant:
  ms                 one call (events around it; the output tiles' allocation is inside, as in the driver)
  vector_tflops      the vector-pipe operations the kernels of sp_fuzzy_step issue -- 3 n k d per distance sweep, of
                     which there are 1 + ceil(d / 128) (+ 1 for U), and 2 n k d for the sums -- / ms; for map2 only the
                     share of its fuzzy_step call is counted, so the figure is a lower bound there
  of_vector_peak     that over the fp32 (157.3 TFLOP/s) or fp64 (78.6) vector peak, which counts an FMA as two: the
                     contract forbids contraction, so a kernel of separate subtract / multiply / add tops out at one half
  nk_bytes           bytes of n x k traffic (U and W written and read) the variant moves and 'fused' does not
Before timing, the first 64 rows of the step are checked against the oracle and the derived bound of the test-suite.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_VECTOR_TFLOPS = {'float32': 157.3, 'float64': 78.6}
SHAPES = {'float32': (1250000, 256, 1024), 'float64': (200000, 64, 256)}
M, SEED, PANEL = 2.0, 20151020, 128
STEP_SECONDS = 420


def _inputs(n, d, k, dtype):
  rng = np.random.default_rng(SEED)
  if dtype == np.dtype(np.float32):
    return rng.random((n, d), dtype=np.float32), rng.random((k, d), dtype=np.float32)
  return rng.random((n, d)), rng.random((k, d))


def _fused(be, x, c):
  return be.fuzzy_step(x, c, M)


def _fused_u(be, x, c):
  return be.fuzzy_step(x, c, M, want_u=True)


def _map2(be, x, c):
  u = be.fuzzy_step(x, c, M, want_u=True)[3]
  labels = u.argmax(axis=1)
  w = u ** x.dtype.type(M)
  return labels, w.T.dot(x), w.sum(axis=0)


VARIANTS = (('fused', _fused), ('fused_u', _fused_u), ('map2', _map2))


def _check(be, x, c):
  from tests import fuzzy_cases
  rows = np.ascontiguousarray(x[:64])
  out = be.fuzzy_step(be.from_numpy(rows), be.from_numpy(c), M, want_u=True)
  fuzzy_cases.check_step(rows, c, M, *(t.numpy() for t in out), label='bench rows')


def step(name, reps):
  import spartan_amd as sp
  from spartan_amd import devarray as D, kernels
  dtype = np.dtype(name)
  n, d, k = SHAPES[name]
  be = sp.initialize('hip', num_workers=1).backend
  x, c = _inputs(n, d, k, dtype)
  _check(be, x, c)
  xt, ct = be.from_numpy(x), be.from_numpy(c)
  for _, fn in VARIANTS:
    fn(be, xt, ct)
  D.synchronize()
  ms = {label: [] for label, _ in VARIANTS}
  for _ in range(reps):
    for label, fn in VARIANTS:
      e0, e1 = kernels.Event(), kernels.Event()
      e0.record()
      out = fn(be, xt, ct)
      e1.record()
      e1.synchronize()
      ms[label].append(e0.elapsed_ms(e1))
      del out
  nkd, nk = float(n) * k * d, float(n) * k * dtype.itemsize
  sweeps = 1 + -(-d // PANEL)
  for label, _ in VARIANTS:
    t = float(np.median(ms[label]))
    ops = (3 * (sweeps + (label != 'fused')) + 2) * nkd
    # U: one write, and for map2 two reads (argmax, **); W: one write and two reads (dot, sum)
    nk_bytes = {'fused': 0.0, 'fused_u': nk, 'map2': 6 * nk}[label]
    print(json.dumps(dict(kernel='fuzzy_step', variant=label, dtype=name, n=n, d=d, k=k, m=M, ms=round(t, 3),
                          ms_min=round(min(ms[label]), 3), ms_max=round(max(ms[label]), 3), reps=reps,
                          distance_sweeps=sweeps + (label != 'fused'), vector_tflops=round(ops / t / 1e9, 2),
                          of_vector_peak=round(ops / t / 1e9 / PEAK_VECTOR_TFLOPS[name], 4),
                          nk_bytes=int(nk_bytes))), flush=True)
  sp.shutdown()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=None)
  ap.add_argument('--step', default=None, help='(internal) run one step in this process')
  args = ap.parse_args()
  if args.step:
    if args.step not in SHAPES:
      raise SystemExit('unknown step %r' % args.step)
    step(args.step, args.reps)
    return
  rows = []
  for name in ('float32', 'float64'):
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', name,
           '--reps', str(args.reps)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    for line in proc.stdout.splitlines():
      print(line, flush=True)
      if line.startswith('{'):
        rows.append(json.loads(line))
    if args.out:
      with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
    if proc.returncode != 0:
      raise SystemExit('bench_fuzzy: step %r ended with status %d; nothing further is started' % (name, proc.returncode))


if __name__ == '__main__':
  main()
