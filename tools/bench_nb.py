"""Times the naive Bayes step of a row tile (sp_nb_step) with HIP events on the library's stream, against the same
result composed from the kernels that were there before it and against a device copy of the tile, on the same build in
the same run.

  python tools/bench_nb.py [--reps 7] [--out profiles/nb_rates.json]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Steps, each in float32 and float64:
  ref    640 000 x 128 documents x terms, 128 labels (the reference's own benchmark, tests/test_naive_bayes.py)
  wide   1 250 000 x 256, 20 labels
Counts 0 .. 7 drawn on the host from a seed (an eighth of them 0), labels uniform.  Per step the variants are warmed up
once each and then timed ALTERNATELY, `reps` rounds; every figure is the median (min and max beside it).  Variants:
  fused     backend.nb_step(x, labels, label_size): S, df and bad; x is read twice, nothing of size n x d is written
  composed  the same S and df from kernels the parent of this change already had, as expressions on one tile:
            df = sum(x > 0, axis=0) and q = sum(x * x, axis=1), each one fused map -> reduce kernel; z = x / sqrt(q / d),
            the map that writes n x d; backend.segment_sum(z, labels, label_size).  The events also see the host
            building and lowering the expressions between the launches, which `fused` does not have: `floor_ms` is the
            time the composition's bytes would take at the copy's measured rate, whatever issues them
  copy      kernels.stream_copy of the tile: n d elements read and n d written
One JSON line per variant:
  ms          one call (events around it; the output tiles' allocation is inside, as in the driver)
  bytes       what the variant must move: fused 2 n d elements + the labels (8 n) + r written and read (2 n elements);
              composed 5 n d elements (x three times, z written and read) + the labels; copy 2 n d elements
  tb_per_s    bytes / ms
  of_copy     tb_per_s over the copy's tb_per_s of the same step (fused and composed)
  floor_ms    (composed) bytes / the copy's rate
and one line `summary` per step: fused_over_composed (ms over ms) and fused_over_composed_floor.
Before timing, the first 64 rows of the step are checked against the oracle and the derived bound of the test-suite,
and the composed S against the fused one (relative to the largest entry; printed as max_rel_diff).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {'ref': (640000, 128, 128), 'wide': (1250000, 256, 20)}
STEPS = tuple((shape, name) for shape in ('ref', 'wide') for name in ('float32', 'float64'))
SEED = 20151123
STEP_SECONDS = 300


def _inputs(n, d, label_size, dtype):
  rng = np.random.default_rng(SEED)
  x = np.floor(rng.random((n, d), dtype=np.float32) * 8).astype(dtype)
  x[:, 0] += 1                                  # no row of zeros
  return x, rng.integers(0, label_size, size=n, dtype=np.int64)


def _check(be, x, labels, label_size):
  from tests import nb_cases
  rows, lab = np.ascontiguousarray(x[:64]), np.ascontiguousarray(labels[:64])
  out = be.nb_step(be.from_numpy(rows), be.from_numpy(lab), label_size)
  nb_cases.check_step(rows, lab, label_size, *(t.numpy() for t in out), label='bench rows')


def step(shape, name, reps):
  import spartan_amd as sp
  from spartan_amd import devarray as D, expr, kernels
  from spartan_amd.array import extent
  dtype = np.dtype(name)
  n, d, label_size = SHAPES[shape]
  be = sp.initialize('hip', num_workers=1).backend
  x, labels = _inputs(n, d, label_size, dtype)
  _check(be, x, labels, label_size)
  X = expr.evaluate(expr.from_numpy(x, tile_hint=(n, d)))
  whole = extent.from_shape((n, d))
  xt, lt = X.fetch(whole), be.from_numpy(labels)
  spare = be.empty((n, d), dtype)
  del x

  def fused():
    return be.nb_step(xt, lt, label_size)

  def composed():
    df = expr.sum(expr.astype(X > 0, np.int64), axis=0).optimized().evaluate()
    q = expr.sum(X * X, axis=1)
    z = (X / expr.reshape(expr.sqrt(q / dtype.type(d)), (n, 1))).optimized().evaluate()
    return be.segment_sum(z.fetch(whole), lt, label_size), df

  def copy():
    return kernels.stream_copy(spare, xt)

  variants = (('fused', fused), ('composed', composed), ('copy', copy))
  a, b = fused()[0].numpy(), composed()[0].numpy()
  max_rel_diff = float(np.abs(a.astype(np.float64) - b).max() / np.abs(a).max())
  copy()
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
  sz = dtype.itemsize
  nd = float(n) * d * sz
  nbytes = {'fused': 2 * nd + 8.0 * n + 2.0 * n * sz, 'composed': 5 * nd + 8.0 * n, 'copy': 2 * nd}
  med = {label: float(np.median(ms[label])) for label, _ in variants}
  rate = {label: nbytes[label] / med[label] / 1e9 for label, _ in variants}       # TB/s
  for label, _ in variants:
    row = dict(kernel='nb_step', shape=shape, variant=label, dtype=name, n=n, d=d, label_size=label_size,
               ms=round(med[label], 3), ms_min=round(min(ms[label]), 3), ms_max=round(max(ms[label]), 3), reps=reps,
               bytes=int(nbytes[label]), tb_per_s=round(rate[label], 3))
    if label != 'copy':
      row['of_copy'] = round(rate[label] / rate['copy'], 4)
    if label == 'composed':
      row['floor_ms'] = round(nbytes[label] / rate['copy'] / 1e9, 3)
      row['max_rel_diff'] = max_rel_diff
    print(json.dumps(row), flush=True)
  floor = nbytes['composed'] / rate['copy'] / 1e9
  print(json.dumps(dict(kernel='nb_step', shape=shape, variant='summary', dtype=name,
                        fused_over_composed=round(med['fused'] / med['composed'], 4),
                        fused_over_composed_floor=round(med['fused'] / floor, 4),
                        fused_bytes_over_composed_bytes=round(nbytes['fused'] / nbytes['composed'], 4))), flush=True)
  sp.shutdown()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--out', default=None)
  ap.add_argument('--step', default=None, help='(internal) run one step in this process: <shape>:<dtype>')
  args = ap.parse_args()
  if args.step:
    shape, _, name = args.step.partition(':')
    if (shape, name) not in STEPS:
      raise SystemExit('unknown step %r' % args.step)
    step(shape, name, args.reps)
    return
  rows = []
  for shape, name in STEPS:
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step',
           '%s:%s' % (shape, name), '--reps', str(args.reps)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    for line in proc.stdout.splitlines():
      print(line, flush=True)
      if line.startswith('{'):
        rows.append(json.loads(line))
    if args.out:
      with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
    if proc.returncode != 0:
      raise SystemExit('bench_nb: step %s:%s ended with status %d; nothing further is started' % (shape, name, proc.returncode))


if __name__ == '__main__':
  main()
