"""Times the swaption path kernel (sp_lmm_swaption) with HIP events on the library's stream, against the reference's
array program on the expression builders of the same build (examples.swaption, method='expr'), against the NumPy tile
body on the host (examples/_swaption.payoffs_numpy), and inside the driver; then the reference's whole benchmark.

  python tools/bench_swaption.py [--reps 7] [--out profiles/swaption_rates.json]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Steps: the product (ts, te, lamb) = (18, 20, 0.1) --
S = 36 steps of K = 40 maturities, 1548 exp per pair of paths -- in float32 and float64 at 10, 65 536 and 2^20 pairs, on
draws made on the host from a seed; then `benchmark`, the 16 products of tests/benchmark_swaption.py at 10 paths in
float64.  Per step the device variants are warmed up once each and then timed ALTERNATELY, `reps` rounds; every figure
is the median (min and max beside it).  Variants of a product step:
  fused         backend.lmm_swaption(eps, 40, 0.1) on draws that are on the device: one launch, HIP events
  copy          backend.copy(eps): the draws read once and written once by the device's copy, HIP events
  driver_fused  examples.swaption.simulate for the one product with eps_all (a distributed array on the device),
                method='fused': the shuffle, the kernel, mean and std, host clock around the call and a synchronisation
  driver_expr   the same call with method='expr' (10 and 65 536 pairs; at 2^20 the plane of 40 x 2^21 values and its
                temporaries are not attempted), `expr_reps` rounds
  numpy         payoffs_numpy on the host on the same draws (10 and 65 536 pairs), timed once with the host clock
One JSON line per variant:
  ms              one call
  exp_per_s       (fused) n * 1548 / ms
  valu_per_exp    (fused) vector instructions per exp evaluation in the kernel's unrolled k loop, read from the ISA of
                  this build's flags (hipcc -S on csrc/lmm.hip: the loop body of 4 maturities, everything between its
                  label and its backward branch, divided by 4: 132 vector instructions per 4 maturities in
                  float32 -- 4 v_exp_f32 and 20 of a division's v_rcp / v_div_* among them --, 170 in float64)
  of_valu_issue   (fused) exp_per_s * valu_per_exp over the chip's vector issue rate, taken -- as tools/bench_nbody.py
                  and tools/bench_cf.py take it -- as 256 CUs x 4 SIMDs x one wave64 float32 instruction per 2 cycles at
                  2.4 GHz = 1228.8 G wave-instructions/s x 64 lanes.  A float64 instruction, a division's and exp's
                  transcendental-rate instructions and the LDS accesses take more than 2 cycles: 1.0 is not reachable.
and one line `summary` per step with expr_over_fused (driver ms over driver ms) where expr ran.  The `benchmark` step
has the two driver variants alone.  Before timing, 64 pairs of the step are checked against the oracle and the derived
bound of the test-suite."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TS, TE, LAMB = 18, 20, 0.1
S, K = 36, 40
EXP_PER_PAIR = 2 * (S * K - S * (S + 1) // 2)
SIZES = (10, 65536, 1 << 20)
EXPR_MAX_N = 65536
STEPS = tuple('%d:%s' % (n, name) for n in SIZES for name in ('float32', 'float64')) + ('benchmark',)
SEED = 20261021
STEP_SECONDS = 280
VALU_PER_EXP = {'float32': 132 / 4.0, 'float64': 170 / 4.0}
WAVE_INSTRUCTIONS_PER_S = 256 * 4 * 2.4e9 / 2


def _row(ms, **kw):
  row = dict(kernel='lmm_swaption', ms=round(float(np.median(ms)), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4),
             reps=len(ms))
  row.update(kw)
  return row


def _host_timed(fn, sync, reps):
  out = []
  for _ in range(reps):
    t0 = time.perf_counter()
    fn()
    sync()
    out.append((time.perf_counter() - t0) * 1e3)
  return out


def product_step(n, name, reps, expr_reps):
  import spartan_amd as sp
  from spartan_amd import devarray as D, kernels
  from spartan_amd.examples import _swaption, swaption
  from tests import swaption_cases as wc
  dtype = np.dtype(name)
  be = sp.initialize('hip', num_workers=1).backend
  eps = np.ascontiguousarray(np.random.default_rng(SEED + n).standard_normal((S, n)).astype(dtype))
  dev = be.from_numpy(eps)
  head = min(n, 64)
  got = be.lmm_swaption(dev[:, :head], K, LAMB).numpy()
  assert wc.share(got, wc.oracle(eps[:, :head], K, LAMB), wc.bound(eps[:, :head], K, LAMB)) <= 1.0

  variants = [('fused', lambda: be.lmm_swaption(dev, K, LAMB)), ('copy', lambda: be.copy(dev))]
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
  dist = sp.from_numpy(eps, tile_hint=(S, n)).evaluate()

  def driver(method):
    r = swaption.simulate([[TS]], [TE], [LAMB], n, method=method, dtype=dtype, eps_all=[dist])
    return float(np.asarray(r[0][0].glom()))
  fused_bp = driver('fused')                            # (warm-up)
  ms['driver_fused'] = _host_timed(lambda: driver('fused'), D.synchronize, reps)
  if n <= EXPR_MAX_N:
    expr_bp = driver('expr')                            # (warm-up)
    assert abs(expr_bp - fused_bp) <= (1e-3 if dtype == np.float32 else 1e-9) * abs(fused_bp), (expr_bp, fused_bp)
    ms['driver_expr'] = _host_timed(lambda: driver('expr'), D.synchronize, expr_reps)
    ms['numpy'] = _host_timed(lambda: _swaption.payoffs_numpy(eps, K, LAMB, 0.5, 0.06, 0.06), lambda: None, 1)
  for label, v in ms.items():
    row = _row(v, variant=label, dtype=name, n=n, steps=S, maturities=K)
    if label == 'fused':
      rate = n * EXP_PER_PAIR / row['ms'] * 1e3
      row.update(exp_per_s=float('%.4g' % rate), valu_per_exp=VALU_PER_EXP[name],
                 of_valu_issue=round(rate * VALU_PER_EXP[name] / (WAVE_INSTRUCTIONS_PER_S * 64), 4))
    print(json.dumps(row), flush=True)
  summary = dict(kernel='lmm_swaption', variant='summary', dtype=name, n=n, mean_bp=round(fused_bp, 3),
                 driver_over_kernel=round(float(np.median(ms['driver_fused']) / np.median(ms['fused'])), 2))
  if 'driver_expr' in ms:
    summary['expr_over_fused'] = round(float(np.median(ms['driver_expr']) / np.median(ms['driver_fused'])), 2)
    summary['numpy_over_kernel'] = round(float(ms['numpy'][0] / np.median(ms['fused'])), 2)
  print(json.dumps(summary), flush=True)
  sp.shutdown()


def benchmark_step(reps):
  import spartan_amd as sp
  from spartan_amd import devarray as D
  from spartan_amd.examples import swaption
  from tests import swaption_cases as wc
  ctx = sp.initialize('hip', num_workers=1)
  sp.set_random_seed(SEED)
  ms, launches = {}, {}
  for method in ('fused', 'expr'):
    def run(method=method):
      return swaption.simulate(wc.TS_ALL, wc.TE_ALL, wc.LAMB_ALL, wc.NUM_PATHS, method=method)
    run()                                               # (warm-up)
    before = ctx.backend.launches
    run()
    D.synchronize()
    launches[method] = ctx.backend.launches - before
    ms[method] = _host_timed(run, D.synchronize, reps)
  for method, v in ms.items():
    print(json.dumps(_row(v, variant='benchmark_' + method, dtype='float64', n=wc.NUM_PATHS, products=16,
                          launches=launches[method])), flush=True)
  print(json.dumps(dict(kernel='lmm_swaption', variant='summary', step='benchmark',
                        expr_over_fused=round(float(np.median(ms['expr']) / np.median(ms['fused'])), 2))), flush=True)
  sp.shutdown()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--expr-reps', type=int, default=3)
  ap.add_argument('--out', default=None)
  ap.add_argument('--step', default=None, help='(internal) run one step in this process: <n>:<dtype> or benchmark')
  args = ap.parse_args()
  if args.step:
    if args.step not in STEPS:
      raise SystemExit('unknown step %r' % args.step)
    if args.step == 'benchmark':
      benchmark_step(args.reps)
    else:
      n, name = args.step.split(':')
      product_step(int(n), name, args.reps, args.expr_reps)
    return
  rows = []
  for step in STEPS:
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', step,
           '--reps', str(args.reps), '--expr-reps', str(args.expr_reps)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    for line in proc.stdout.splitlines():
      print(line, flush=True)
      if line.startswith('{'):
        rows.append(json.loads(line))
    if args.out:
      with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
    if proc.returncode != 0:
      raise SystemExit('bench_swaption: step %s ended with status %d; nothing further is started' % (step, proc.returncode))


if __name__ == '__main__':
  main()
