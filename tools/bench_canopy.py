"""Times the canopy kernels (sp_canopy, sp_pdf_label) with HIP events on the library's stream, against the NumPy tile
bodies on the host (examples/_canopy.py: the loops the reference runs per tile), against the same labels composed from
the existing kernels, and inside the whole canopy_cluster call.

  python tools/bench_canopy.py [--reps 7] [--out profiles/canopy_rates.json]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Per step the variants are warmed up once each and then
timed ALTERNATELY, `reps` rounds; every figure is the median (min and max beside it).  Steps, each in float64 and
float32 on points drawn on the host from a seed:
  tile      240 000 x 2 uniform in the unit square, t1 = t2 = 0.1: one tile of the reference's tests/
            test_canopy_clustering.py (30 000 x 64 points at 8 workers)
              kernel_chains_<c>  kernels.canopy into targets made beforehand, c = 1, 64, 1024: the one launch
              call_chains_<c>    backend.canopy: the launch, the wait for the counts and the copies to the host (host clock)
              numpy              canopy_numpy on the host on the same tile, one chain, timed once with the host clock
  many      16 384 x 16 uniform in the unit cube, t1 = 0.96, t2 = 0.8 (a few thousand canopies), cap = n: the same
            variants with c = 1, 16, 256
  small     40, 160, 640, 2560 and 10 240 x 2 of the same points: call_chains_1 (backend.canopy, host clock) against
            numpy (canopy_numpy, the median of `reps` runs): where the host loop wins
  label     pdf_label of 240 000 x 2 among the tile's own centres and of 1 250 000 x 256 among 1024 centres:
              pdf_label   backend.pdf_label: one launch
              knn_1       backend.knn(x, centres, 1): the nearest centre from the existing kernel (its index equals the
                          label wherever no two pdfs tie after rounding; the share of equal labels is reported)
              numpy       (the small shape only) pdf_label_numpy on the host, timed once
  cluster   the whole canopy_cluster call on 1 920 000 x 2 at 8 logical workers, labels forced, with the host clock
            around the call and a device synchronisation: chains_per_tile = 1, 64 and 1024
One JSON line per variant:
  ms               one call
  rows_per_s       n / ms
  us_per_block     (kernel_chains_<c>) the time of one chain's block of 64 rows: ms * c / ceil(n / 64)
  canopies         (kernel_chains_<c>) the canopies of all chains
Before timing, the step's results are checked byte for byte against the NumPy bodies on its first rows."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DTYPES = ('float64', 'float32')
STEPS = tuple((kind, name) for kind in ('tile', 'many', 'small', 'label', 'cluster') for name in DTYPES)
SEED = 20261021
STEP_SECONDS = 280
TILE = dict(n=240000, d=2, t1=0.1, t2=0.1, chains=(1, 64, 1024))
MANY = dict(n=16384, d=16, t1=0.96, t2=0.8, chains=(1, 16, 256))


def _median_rows(kernel, name, ms, extra):
  for label, v in ms.items():
    row = dict(kernel=kernel, variant=label, dtype=name, ms=round(float(np.median(v)), 4), ms_min=round(min(v), 4),
               ms_max=round(max(v), 4), reps=len(v))
    row.update(extra(label, float(np.median(v))))
    print(json.dumps(row), flush=True)


def _timed(variants, reps, clock):
  """{label: [ms]} of the variants timed alternately; clock(fn) -> ms."""
  for _, fn in variants:
    fn()
  ms = {label: [] for label, _ in variants}
  for _ in range(reps):
    for label, fn in variants:
      ms[label].append(clock(fn))
  return ms


def _clocks():
  from spartan_amd import devarray as D, kernels

  def events(fn):
    e0, e1 = kernels.Event(), kernels.Event()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_ms(e1)

  def host(fn):
    D.synchronize()
    t0 = time.perf_counter()
    out = fn()
    D.synchronize()
    del out
    return (time.perf_counter() - t0) * 1e3
  return events, host


def canopy_step(kind, name, reps):
  import spartan_amd as sp
  from spartan_amd import kernels
  from spartan_amd.examples import _canopy
  p = TILE if kind == 'tile' else MANY
  n, d, t1, t2 = p['n'], p['d'], p['t1'], p['t2']
  dtype = np.dtype(name)
  be = sp.initialize('hip', num_workers=1).backend
  events, host = _clocks()
  x = np.random.default_rng(SEED + n).random((n, d)).astype(dtype)
  dev = be.from_numpy(x)
  got = be.canopy(dev[:3000], t1, t2, chains=2)
  want = _canopy.canopy_numpy(x[:3000], t1, t2, 2)
  assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))

  variants, canopies = [], {}
  for c in p['chains']:
    cap = -(-n // c) if kind == 'many' else min(-(-n // c), 1024)
    targets = (be.empty((c * cap, d), dtype), be.empty((c * cap,), np.int64), be.empty((c * cap,), np.int64),
               be.empty((c,), np.int64))
    variants.append(('kernel_chains_%d' % c, (lambda c=c, cap=cap, t=targets: kernels.canopy(dev, t1, t2, c, cap, *t))))
    kernels.canopy(dev, t1, t2, c, cap, *targets)
    num = targets[3].numpy()
    assert (num >= 0).all()
    canopies[c] = int(num.sum())
  ms = _timed(variants, reps, events)
  ms.update(_timed([('call_chains_%d' % c, (lambda c=c: be.canopy(dev, t1, t2, chains=c,
                                                                  cap=-(-n // c) if kind == 'many' else None)))
                    for c in p['chains']], reps, host))
  t0 = time.perf_counter()
  ref = _canopy.canopy_numpy(x, t1, t2, 1)
  ms['numpy'] = [(time.perf_counter() - t0) * 1e3]
  assert len(ref[0]) == canopies[1]

  def extra(label, med):
    out = dict(n=n, d=d, t1=t1, t2=t2, rows_per_s=float('%.4g' % (n / med * 1e3)))
    if label.startswith('kernel_chains_'):
      c = int(label.rsplit('_', 1)[1])
      out.update(us_per_block=float('%.4g' % (med * 1e3 * c / -(-n // 64))), canopies=canopies[c])
    if label == 'numpy':
      out['canopies'] = canopies[1]
    return out
  _median_rows('canopy_' + kind, name, ms, extra)
  sp.shutdown()


def small_step(name, reps):
  import spartan_amd as sp
  from spartan_amd.examples import _canopy
  dtype = np.dtype(name)
  be = sp.initialize('hip', num_workers=1).backend
  _, host = _clocks()
  t1, t2 = TILE['t1'], TILE['t2']
  for n in (40, 160, 640, 2560, 10240):
    x = np.random.default_rng(SEED + TILE['n']).random((n, TILE['d'])).astype(dtype)
    dev = be.from_numpy(x)
    want = _canopy.canopy_numpy(x, t1, t2, 1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(be.canopy(dev, t1, t2), want))
    ms = _timed([('call_chains_1', lambda: be.canopy(dev, t1, t2))], reps, host)
    ms['numpy'] = []
    for _ in range(reps):
      t0 = time.perf_counter()
      _canopy.canopy_numpy(x, t1, t2, 1)
      ms['numpy'].append((time.perf_counter() - t0) * 1e3)
    _median_rows('canopy_small', name, ms, lambda label, med: dict(
        n=n, d=TILE['d'], t1=t1, t2=t2, canopies=len(want[0]), rows_per_s=float('%.4g' % (n / med * 1e3))))
  sp.shutdown()


def label_step(name, reps):
  import spartan_amd as sp
  from spartan_amd.examples import _canopy
  dtype = np.dtype(name)
  be = sp.initialize('hip', num_workers=1).backend
  events, _ = _clocks()
  rng = np.random.default_rng(SEED)
  small = rng.random((TILE['n'], TILE['d'])).astype(dtype)
  centres, counts, _ = _canopy.canopy_numpy(small[:20000], TILE['t1'], TILE['t2'], 1)
  centres = np.ascontiguousarray(centres[counts > 1])
  for x, c in ((small, centres), (None, None)):
    if x is None:
      n, d, k = 1250000, 256, 1024
      x = rng.random((n, d), dtype=np.float32).astype(dtype, copy=False)
      c = rng.random((k, d)).astype(dtype)
    n, d, k = x.shape[0], x.shape[1], c.shape[0]
    xd, cd = be.from_numpy(x), be.from_numpy(c)
    got = be.pdf_label(xd, cd).numpy()
    assert got[:2000].tobytes() == _canopy.pdf_label_numpy(x[:2000], c).tobytes()
    agree = float((be.knn(xd, cd, 1)[1].numpy().reshape(n) == got).mean())
    ms = _timed([('pdf_label', lambda: be.pdf_label(xd, cd)), ('knn_1', lambda: be.knn(xd, cd, 1))], reps, events)
    if n == TILE['n']:
      t0 = time.perf_counter()
      _canopy.pdf_label_numpy(x, c)
      ms['numpy'] = [(time.perf_counter() - t0) * 1e3]
    _median_rows('pdf_label', name, ms, lambda label, med: dict(
        n=n, d=d, k=k, rows_per_s=float('%.4g' % (n / med * 1e3)),
        gflops=float('%.4g' % (3.0 * n * k * d / med * 1e-6)), **({'labels_equal': agree} if label == 'knn_1' else {})))
    del xd, cd
  sp.shutdown()


def cluster_step(name, reps):
  import spartan_amd as sp
  from spartan_amd import expr
  from spartan_amd.examples import canopy_clustering as cc
  dtype = np.dtype(name)
  sp.initialize('hip', num_workers=8)
  _, host = _clocks()
  n, d = 30000 * 64, 2
  x = np.random.default_rng(SEED + 1).random((n, d)).astype(dtype)
  pts = expr.from_numpy(x, tile_hint=(n // 8, d)).evaluate()
  found = {}

  def run(chains):
    labels, centres = cc.canopy_cluster(pts, chains_per_tile=chains, return_centers=True)
    found[chains] = len(centres)
    return labels.force()
  ms = _timed([('chains_per_tile_%d' % c, (lambda c=c: run(c))) for c in TILE['chains']], reps, host)
  _median_rows('canopy_cluster', name, ms, lambda label, med: dict(
      n=n, d=d, workers=8, centres=found[int(label.rsplit('_', 1)[1])], rows_per_s=float('%.4g' % (n / med * 1e3))))
  sp.shutdown()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=7)
  ap.add_argument('--out', default=None)
  ap.add_argument('--step', default=None, help='(internal) run one step in this process: <kind>:<dtype>')
  args = ap.parse_args()
  if args.step:
    kind, name = args.step.split(':')
    if (kind, name) not in STEPS:
      raise SystemExit('unknown step %r' % args.step)
    if kind in ('tile', 'many'):
      canopy_step(kind, name, args.reps)
    elif kind == 'small':
      small_step(name, args.reps)
    elif kind == 'label':
      label_step(name, args.reps)
    else:
      cluster_step(name, args.reps)
    return
  rows = []
  for kind, name in STEPS:
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step',
           '%s:%s' % (kind, name), '--reps', str(args.reps)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
    for line in proc.stdout.splitlines():
      print(line, flush=True)
      if line.startswith('{'):
        rows.append(json.loads(line))
    if args.out:
      with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
    if proc.returncode != 0:
      raise SystemExit('bench_canopy: step %s:%s ended with status %d; nothing further is started' % (kind, name, proc.returncode))


if __name__ == '__main__':
  main()
