"""Times the dual coordinate ascent kernel (sp_svm_dca) with HIP events on the library's stream, against the NumPy tile
body on the host (examples/_svm.dca_numpy: the loop the reference runs per tile), against a device copy of the same
bytes, and inside a whole iteration of the driver.

  python tools/bench_svm.py [--reps 7] [--out profiles/svm_rates.json]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Steps, each in float64 and float32 on rows of norm
about 1 with labels from a noisy hyperplane (drawn on the host from a seed), alpha = 0, w0 = 0, scaled_lambda = 1:
  64000 x 64 (the reference's tests/test_svm.py) and 8192 x 1024, one pass over the rows.
Per step the variants are warmed up once each and then timed ALTERNATELY, `reps` rounds; every figure is the median
(min and max beside it).  Variants:
  chains_<c>   backend.svm_dca(x, y, alpha, w0, 1.0, chains=c), c = 1, 8, 64, 256, 1024: one launch
  copy         backend.copy(x): the same bytes read once and written once by the device's copy
  numpy        dca_numpy on the host on the same operands, chains = 1, timed once with the host clock
  fit_iter     (64000 x 64 only) one iteration of examples.disdca_svm.fit_state at 1 worker and chains_per_tile = 64 --
               the pass, the host's copy of w and the expression for w -- as (T = 3 minus T = 1) / 2 with the host
               clock around the call and a device synchronisation
One JSON line per variant:
  ms              one call
  rows_per_s      m / ms
  ns_per_row      (chains_<c>) the time of one chain's row: ms * c / m -- with one chain the latency of a row's
                  critical path (B's cross-lane tree, one division, the broadcast-free update)
  of_copy         (chains_<c>) the bytes of X per second over the copy's bytes READ per second
Before timing, the first 300 rows of the step are checked byte for byte against dca_numpy."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((64000, 64), (8192, 1024))
STEPS = tuple((m, d, name) for m, d in SHAPES for name in ('float64', 'float32'))
CHAINS = (1, 8, 64, 256, 1024)
SEED = 20261020
STEP_SECONDS = 280


def _inputs(m, d, dtype):
  rng = np.random.default_rng(SEED + m + d)
  x = (rng.standard_normal((m, d)) / np.sqrt(d)).astype(dtype)
  truth = rng.standard_normal(d)
  y = np.where(x.astype(np.float64).dot(truth) + 0.1 * rng.standard_normal(m) >= 0, 1, -1).astype(dtype)
  return x, y, np.zeros(m, dtype), np.zeros(d, dtype)


def step(m, d, name, reps):
  import spartan_amd as sp
  from spartan_amd import devarray as D, kernels
  from spartan_amd.examples import _svm, disdca_svm
  dtype = np.dtype(name)
  be = sp.initialize('hip', num_workers=1).backend
  x, y, alpha, w0 = _inputs(m, d, dtype)
  dev = [be.from_numpy(v) for v in (x, y, alpha, w0)]
  got = be.svm_dca(dev[0][:300], dev[1][:300], dev[2][:300], dev[3], 1.0, chains=2, want_w=True)
  want = _svm.dca_numpy(x[:300], y[:300], alpha[:300], w0, 1.0, 2)
  assert got[0].numpy().tobytes() == want[0].tobytes() and got[1].numpy().tobytes() == want[1].tobytes()

  variants = [('chains_%d' % c, (lambda c=c: be.svm_dca(*dev, 1.0, chains=c))) for c in CHAINS]
  variants.append(('copy', lambda: be.copy(dev[0])))
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
  t0 = time.perf_counter()
  _svm.dca_numpy(x, y, alpha, w0, 1.0, 1)
  ms['numpy'] = [(time.perf_counter() - t0) * 1e3]
  if (m, d) == SHAPES[0]:
    def fit(iters):
      t0 = time.perf_counter()
      disdca_svm.fit_state(x, y, T=iters, la=1.0, chains_per_tile=64)
      D.synchronize()
      return (time.perf_counter() - t0) * 1e3
    fit(1)                                              # (warm-up)
    ms['fit_iter'] = [(fit(3) - fit(1)) / 2 for _ in range(reps)]
  med = {label: float(np.median(v)) for label, v in ms.items()}
  copy_read = x.nbytes / med['copy']
  for label in ms:
    row = dict(kernel='svm_dca', variant=label, dtype=name, m=m, d=d, ms=round(med[label], 4),
               ms_min=round(min(ms[label]), 4), ms_max=round(max(ms[label]), 4), reps=len(ms[label]))
    if label != 'copy':
      row['rows_per_s'] = float('%.4g' % (m / med[label] * 1e3))
    if label.startswith('chains_'):
      c = int(label.split('_')[1])
      row['ns_per_row'] = float('%.4g' % (med[label] * 1e6 * c / m))
      row['of_copy'] = round(x.nbytes / med[label] / copy_read, 4)
    if label == 'copy':
      row['read_gb_per_s'] = float('%.4g' % (copy_read * 1e-6))
    print(json.dumps(row), flush=True)
  best = min(CHAINS, key=lambda c: med['chains_%d' % c])
  print(json.dumps(dict(kernel='svm_dca', variant='summary', dtype=name, m=m, d=d, best_chains=best,
                        numpy_over_one_chain=round(med['numpy'] / med['chains_1'], 2),
                        one_chain_over_best=round(med['chains_1'] / med['chains_%d' % best], 2))), flush=True)
  sp.shutdown()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--out', default=None)
  ap.add_argument('--step', default=None, help='(internal) run one step in this process: <m>:<d>:<dtype>')
  args = ap.parse_args()
  if args.step:
    m, d, name = args.step.split(':')
    if (int(m), int(d), name) not in STEPS:
      raise SystemExit('unknown step %r' % args.step)
    step(int(m), int(d), name, args.reps)
    return
  rows = []
  for m, d, name in STEPS:
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step',
           '%d:%d:%s' % (m, d, name), '--reps', str(args.reps)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    for line in proc.stdout.splitlines():
      print(line, flush=True)
      if line.startswith('{'):
        rows.append(json.loads(line))
    if args.out:
      with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
    if proc.returncode != 0:
      raise SystemExit('bench_svm: step %d:%d:%s ended with status %d; nothing further is started' % (m, d, name, proc.returncode))


if __name__ == '__main__':
  main()
