"""Times the affinity kernels of spectral clustering (sp_affinity_degree, sp_affinity_matrix) with HIP events on the
library's stream, against the time to write the matrix at all and against the same quantities phrased with the kernels
the library had before them, on the same build in the same run.

  python tools/bench_spectral.py [--reps 5] [--out profiles/spectral_rates.json]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Steps: n8192 and n32768 points, each with d = 2, 16 and
64 features in float32 and float64, 'rbf' with gamma = 1 / d (points uniform in [0, 1)^d: t = gamma d2 <= 1).  Per
configuration the variants are warmed up once each and then timed ALTERNATELY, `reps` rounds; every figure is the median
(min and max beside it).  Variants:
  degree       backend.affinity_degree(P, P): D [n]; nothing of size n x n exists
  matrix       backend.affinity_matrix(P, 0, P, scale=s): L [n, n], written once
  fill         a tile of n x n elements filled with a constant by the library's own fill kernel: the time to write
               n * n * sizeof(T) bytes on this box, the floor of `matrix`
  composition  the same D and L with the kernels that were here before: |p|^2 by a map and a row reduction, P . P^T by
               the GEMM, d2 = |p_i|^2 + |p_j|^2 - 2 P . P^T and exp(-gamma d2) by map kernels, D by a row reduction,
               L = A s_i s_j by a map kernel -- four passes over n x n (the diagonal is not set to 1: one more)
One JSON line per variant:
  ms                 one call (events around it; the output tile's allocation is inside, as in the driver)
  gbytes_per_s       for matrix and fill: n * n * sizeof(T) / ms
  of_fill            for matrix: fill's ms over matrix's ms
  vector_tflops      for degree and matrix: 3 n^2 d (a subtract, a multiply and an add per pair and feature) / ms
  composition_over_fused   for composition: its ms over degree's + matrix's
Before timing, at n = 8192, the fused L and the composition's are compared on the first 64 rows (the composition's
GEMM-form distance cancels where points are close, so the comparison is absolute: 1e-4 in float32, 1e-12 in float64).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {'n8192': 8192, 'n32768': 32768}
DIMS = (2, 16, 64)
DTYPES = ('float32', 'float64')
SEED = 20151102
STEP_SECONDS = 540


def _scale(deg):
  s = np.sqrt(deg)
  s[s == 0] = 1
  return (1.0 / s).astype(deg.dtype)


def _degree(be, p, s, gamma):
  return be.affinity_degree(p, p, 'rbf', gamma)


def _matrix(be, p, s, gamma):
  return be.affinity_matrix(p, 0, p, 'rbf', gamma, scale=s)


def _fill(be, p, s, gamma):
  from spartan_amd import devarray
  n = p.shape[0]
  return devarray.full((n, n), 1.0, be.dtype_of(p))


def _composition(be, p, s, gamma):
  """(D, L) with map, reduce and GEMM kernels only."""
  n = p.shape[0]
  t = be.dtype_of(p).type
  sq = (p * p).sum(axis=1)
  d2 = sq.reshape(n, 1) + sq.reshape(1, n) - p.dot(p.T) * t(2)
  a = np.exp(d2 * t(-gamma))
  return a.sum(axis=1), a * s.reshape(n, 1) * s.reshape(1, n)


VARIANTS = (('degree', _degree), ('matrix', _matrix), ('fill', _fill), ('composition', _composition))


def _check(be, pt, st, gamma, dtype):
  fused = _matrix(be, pt, st, gamma).numpy()[:64]
  comp = _composition(be, pt, st, gamma)[1].numpy()[:64]
  comp[np.arange(64), np.arange(64)] = 1
  err = float(np.abs(fused - comp).max())
  limit = 1e-4 if dtype == 'float32' else 1e-12
  print('bench_spectral: fused and composed L differ by %.3g absolute (limit %.3g)' % (err, limit), flush=True)
  assert err <= limit


def step(name, reps):
  import spartan_amd as sp
  from spartan_amd import devarray as D, kernels
  n = STEPS[name]
  be = sp.initialize('hip', num_workers=1).backend
  for dtype in DTYPES:
    for d in DIMS:
      gamma = 1.0 / d
      p = np.random.default_rng(SEED).random((n, d)).astype(dtype)
      pt = be.from_numpy(p)
      st = be.from_numpy(_scale(_degree(be, pt, None, gamma).numpy()))
      if n <= 8192:
        _check(be, pt, st, gamma, dtype)
      for _, fn in VARIANTS:
        fn(be, pt, st, gamma)
      D.synchronize()
      ms = {label: [] for label, _ in VARIANTS}
      for _ in range(reps):
        for label, fn in VARIANTS:
          e0, e1 = kernels.Event(), kernels.Event()
          e0.record()
          out = fn(be, pt, st, gamma)
          e1.record()
          e1.synchronize()
          ms[label].append(e0.elapsed_ms(e1))
          del out
      med = {label: float(np.median(ms[label])) for label, _ in VARIANTS}
      nbytes = n * n * np.dtype(dtype).itemsize
      for label, _ in VARIANTS:
        t = med[label]
        row = dict(kernel='affinity', variant=label, dtype=dtype, n=n, d=d, metric='rbf', ms=round(t, 3),
                   ms_min=round(min(ms[label]), 3), ms_max=round(max(ms[label]), 3), reps=reps)
        if label in ('degree', 'matrix'):
          row['vector_tflops'] = round(3.0 * n * n * d / t / 1e9, 2)
        if label in ('matrix', 'fill'):
          row['gbytes_per_s'] = round(nbytes / t / 1e6, 1)
        if label == 'matrix':
          row['of_fill'] = round(med['fill'] / t, 4)
        if label == 'composition':
          row['composition_over_fused'] = round(t / (med['degree'] + med['matrix']), 3)
          row['nn_bytes'] = 4 * nbytes
        print(json.dumps(row), flush=True)
      del pt, st
  sp.shutdown()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=None)
  ap.add_argument('--steps', default='n8192,n32768')
  ap.add_argument('--step', default=None, help='(internal) run one step in this process')
  args = ap.parse_args()
  if args.step:
    if args.step not in STEPS:
      raise SystemExit('unknown step %r' % args.step)
    step(args.step, args.reps)
    return
  rows = []
  for name in args.steps.split(','):
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
      raise SystemExit('bench_spectral: step %r ended with status %d; nothing further is started' % (name, proc.returncode))


if __name__ == '__main__':
  main()
