"""Times the all-pairs gravity kernel (sp_nbody_accel) with HIP events on the library's stream, against the reference's
n x n expression on the map and reduce kernels of the same build in the same run, and against the vector pipe's issue
rate.

  python tools/bench_nbody.py [--reps 7] [--out profiles/nbody_rates.json]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Steps, each in float32 and float64 on a unit-scale
galaxy (positions in the unit cube, masses 0.5 .. 1.5, g = 1, rmin = 0.05; drawn on the host from a seed):
  n = 1000 (the reference's benchmark_nbody.py), 8192 and 65536, the whole array as one band of targets.
Per step the variants are warmed up once each and then timed ALTERNATELY, `reps` rounds; every figure is the median
(min and max beside it).  Variants:
  fused   backend.nbody_accel(x, y, z, mass, 0, n): the three accelerations, nothing of size n x n
  expr    examples.nbody._accel_expr, the reference's expression with the element-wise diagonal, its three sums
          evaluated one after the other through the optimiser (map -> reduce fusion); only where its n x n
          intermediates fit, n <= 8192.  The events also see the host building and lowering the expressions.
At n = 1000 two more: `move_fused` and `move_expr`, one examples.nbody.move end to end (host clock around the call and
a device synchronisation), so that the host's share beside the kernel alone is visible.
One JSON line per variant:
  ms              one call
  pairs_per_s     n * n / ms  (fused and expr)
  valu_per_pair   (fused) vector instructions per pair in the kernel's inner loop, read from the ISA of this build's
                  flags (hipcc -S on csrc/nbody.hip, the loop without the i == j selection: 172 instructions per 4
                  pairs in float32, 201 in float64; two of each pair's are transcendental-rate: sqrt / rsq and rcp)
  of_valu_issue   (fused) pairs_per_s * valu_per_pair over the chip's vector issue rate, taken as 256 CUs x 4 SIMDs x
                  one wave64 float32 instruction per 2 cycles (the measured throughput of v_fma_f32 with several waves
                  per SIMD) at 2.4 GHz = 1228.8 G wave-instructions/s x 64 lanes.  A float64 or transcendental
                  instruction takes more than 2 cycles, so 1.0 is not reachable; the clock under load is below
                  2.4 GHz as well.
and one line `summary` per step with fused_over_expr (ms over ms) where expr ran.
Before timing, 64 targets of the step are checked against the oracle and the derived bound of the test-suite."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1000, 8192, 65536)
EXPR_MAX_N = 8192
STEPS = tuple((n, name) for n in SIZES for name in ('float32', 'float64'))
SEED = 20261020
STEP_SECONDS = 240
G, RMIN = 1.0, 0.05
VALU_PER_PAIR = {'float32': 172 / 4.0, 'float64': 201 / 4.0}
WAVE_INSTRUCTIONS_PER_S = 256 * 4 * 2.4e9 / 2


def _inputs(n, dtype):
  rng = np.random.default_rng(SEED + n)
  x, y, z = (rng.uniform(0.0, 1.0, n).astype(dtype) for _ in range(3))
  return x, y, z, rng.uniform(0.5, 1.5, n).astype(dtype)


def _check(be, x, y, z, mass):
  from tests import nbody_cases as nc
  n = len(x)
  r0 = max(0, n // 2 - 32)
  m = min(64, n - r0)
  out = be.nbody_accel(*(be.from_numpy(v) for v in (x, y, z, mass)), r0, m, g=G, rmin=RMIN)
  # (the bound only: at these sizes a pair may sit within rounding of rmin, which the bound's text discusses)
  nc.check_accel([t.numpy() for t in out], x, y, z, mass, G, RMIN, 'bench targets %d .. %d of %d' % (r0, r0 + m, n),
                 targets=range(r0, r0 + m))


def step(n, name, reps):
  import spartan_amd as sp
  from spartan_amd import devarray as D, expr, kernels
  from spartan_amd.examples import nbody
  dtype = np.dtype(name)
  be = sp.initialize('hip', num_workers=1).backend
  host = _inputs(n, dtype)
  _check(be, *host)
  dev = [be.from_numpy(v) for v in host]
  arrays = [expr.evaluate(expr.from_numpy(v, tile_hint=(n,))) for v in host]

  def fused():
    return be.nbody_accel(*dev, 0, n, g=G, rmin=RMIN)

  def as_expr():
    sums = nbody._accel_expr(*arrays, n, dtype, G, RMIN)
    return [s.optimized().evaluate() for s in sums]

  def galaxy():
    zero = np.zeros(n, dtype)
    return {k: expr.evaluate(expr.from_numpy(v, tile_hint=(n,)))
            for k, v in zip(('x', 'y', 'z', 'm', 'vx', 'vy', 'vz'), host + (zero, zero.copy(), zero.copy()))}

  variants = [('fused', fused)]
  if n <= EXPR_MAX_N:
    variants.append(('expr', as_expr))
  for _, fn in variants:
    fn()
  D.synchronize()
  ms = {label: [] for label, _ in variants}
  for _ in range(reps):
    for label, fn in variants:
      e0, e1 = kernels.Event(), kernels.Event()
      e0.record()
      out = fn()
      e1.record()
      e1.synchronize()
      ms[label].append(e0.elapsed_ms(e1))
      del out
  if n == 1000:
    for method in nbody.METHODS:
      g = galaxy()
      nbody.move(g, 1e-3, method=method, g=G, rmin=RMIN)          # (warm-up)
      D.synchronize()
      ms['move_' + method] = []
      for _ in range(reps):
        t0 = time.perf_counter()
        nbody.move(g, 1e-3, method=method, g=G, rmin=RMIN)
        D.synchronize()
        ms['move_' + method].append((time.perf_counter() - t0) * 1e3)
  med = {label: float(np.median(v)) for label, v in ms.items()}
  for label in ms:
    row = dict(kernel='nbody_accel', variant=label, dtype=name, n=n, ms=round(med[label], 4),
               ms_min=round(min(ms[label]), 4), ms_max=round(max(ms[label]), 4), reps=reps)
    if label in ('fused', 'expr'):
      row['pairs_per_s'] = float('%.4g' % (float(n) * n / med[label] * 1e3))
    if label == 'fused':
      row['valu_per_pair'] = VALU_PER_PAIR[name]
      row['of_valu_issue'] = round(row['pairs_per_s'] * VALU_PER_PAIR[name] / (WAVE_INSTRUCTIONS_PER_S * 64), 4)
    print(json.dumps(row), flush=True)
  summary = dict(kernel='nbody_accel', variant='summary', dtype=name, n=n)
  if 'expr' in med:
    summary['fused_over_expr'] = round(med['fused'] / med['expr'], 4)
  if 'move_fused' in med:
    summary['move_fused_over_move_expr'] = round(med['move_fused'] / med['move_expr'], 4)
    summary['kernel_share_of_move_fused'] = round(med['fused'] / med['move_fused'], 4)
  print(json.dumps(summary), flush=True)
  sp.shutdown()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--out', default=None)
  ap.add_argument('--step', default=None, help='(internal) run one step in this process: <n>:<dtype>')
  args = ap.parse_args()
  if args.step:
    n, _, name = args.step.partition(':')
    if (int(n), name) not in STEPS:
      raise SystemExit('unknown step %r' % args.step)
    step(int(n), name, args.reps)
    return
  rows = []
  for n, name in STEPS:
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step',
           '%d:%s' % (n, name), '--reps', str(args.reps)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    for line in proc.stdout.splitlines():
      print(line, flush=True)
      if line.startswith('{'):
        rows.append(json.loads(line))
    if args.out:
      with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
    if proc.returncode != 0:
      raise SystemExit('bench_nbody: step %d:%s ended with status %d; nothing further is started' % (n, name, proc.returncode))


if __name__ == '__main__':
  main()
