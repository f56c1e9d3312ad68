"""Times the SGD matrix factorisation kernel (sp_sgd_mf) with HIP events on the library's stream against the library's
own plain loop on the host (sp_sgd_mf_host, single-threaded, the same operands): one process, every variant warmed up
once and then timed ALTERNATELY, `reps` rounds; every figure is the median (min and max beside it).

  python tools/bench_netflix.py [--reps 5] [--out profiles/netflix_rates.json]

Tiles: `bench`, one of the 8 x 8 blocks of the reference's tests/benchmark_netflix.py (17770 x 2649429 at 1e8 ratings:
2221 x 331000 with 1.56 M distinct cells drawn uniformly from a seed), at ranks 25 and 50; `golden`, 13 x 100 with the
density of tests/golden/netflix_w4.npz (about 90 ratings), at rank 20; `narrow`, 13 x 1250 with about 975 ratings (about
125 levels of 8: narrow levels only), at rank 20.  All in float32 and float64.
Variants per tile, rank and dtype:
  wide_<w>   the tile's level schedule cut into segments with <w> in the place of SP_MF_WIDE (the tool rewrites the
             segment table of the plan; the entries and levels are the library's): w = 1 makes every level a launch of
             its own, the largest w puts every level into one workgroup.  wide_<SP_MF_WIDE> is the plan as the library
             builds it.
  host       sp_sgd_mf_host in tile order on the host, timed with the host clock (fewer rounds: it is slow)
One JSON line per variant: ms, ratings_per_s, launches, levels, us_per_level (ms / levels), ns_per_rating; and
`plan_ms` once per tile (building the schedule on the host, paid once per tile).  Before timing, one pass of the
library's plan is checked byte for byte against the host loop."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20261021
TILES = {'bench': (2221, 331000, 1560000, (25, 50)), 'golden': (13, 100, 90, (20,)), 'narrow': (13, 1250, 1000, (20,))}
WIDES = (1, 16, 64, 256, 1024, 1 << 30)


def make_tile(m, n, nnz, dtype):
  rng = np.random.default_rng(SEED + m)
  cells = np.unique(rng.integers(0, m * n, nnz))
  rows, cols = cells // n, cells % n
  indptr = np.zeros(m + 1, np.int64)
  np.add.at(indptr, rows + 1, 1)
  return np.cumsum(indptr), cols.astype(np.int32), rng.integers(1, 6, len(cells)).astype(dtype)


def resegment(plan, wide):
  """A copy of a plan (uint8 array) whose segment table is cut with `wide` in the place of SP_MF_WIDE."""
  from spartan_amd import kernels
  parts = kernels.sgd_mf_plan_parts(plan)
  widths = np.diff(parts['level_off'])
  segs = []
  for v, w in enumerate(widths.tolist()):
    if w >= wide:
      segs.append([1, v, v + 1, 0])
    elif segs and segs[-1][0] == 0:
      segs[-1][2] = v + 1
    else:
      segs.append([0, v, v + 1, 0])
  head = plan[:128].view(np.int64).copy()
  off = int(head[11])
  table = np.asarray(segs, np.int32).reshape(-1, 4)
  head[5], head[6] = len(segs), off + table.nbytes
  out = np.empty((off + table.nbytes + 7) // 8, np.int64).view(np.uint8)[:off + table.nbytes]
  out[:off] = plan[:off]
  out[:128] = head.view(np.uint8)
  out[off:] = table.reshape(-1).view(np.uint8)
  return out


def run(be, name, f, dtype, reps, emit):
  from spartan_amd import _hip, devarray as D, kernels
  m, n, nnz, _ = TILES[name]
  dt = np.dtype(dtype)
  indptr, indices, vals = make_tile(m, n, nnz, dt)
  nnz = len(indices)
  rng = np.random.default_rng(SEED + f)
  u0 = ((rng.random((m, f)) + 0.5) / np.sqrt(f)).astype(dt)
  m0 = ((rng.random((n, f)) + 0.5) / np.sqrt(f)).astype(dt)
  t0 = time.perf_counter()
  plan = kernels.sgd_mf_plan(m, n, indptr, indices)
  plan_ms = (time.perf_counter() - t0) * 1e3
  parts = kernels.sgd_mf_plan_parts(plan)
  levels, widths = parts['levels'], np.diff(parts['level_off'])
  base = dict(kernel='sgd_mf', tile=name, m=m, n=n, nnz=nnz, f=f, dtype=dt.name, levels=levels)
  emit(dict(base, variant='plan', plan_ms=round(plan_ms, 3), width_mean=round(float(widths.mean()), 1),
            width_max=int(widths.max()), levels_below_16=int((widths < 16).sum()), levels_below_64=int((widths < 64).sum())))

  dvals = be.from_numpy(vals)
  # one pass of the library's plan against the host loop, byte for byte
  ud, md = be.from_numpy(u0), be.from_numpy(m0)
  kernels.sgd_mf((m, n), dvals, be.from_numpy(plan), plan, ud, md)
  hu, hm = u0.copy(), m0.copy()
  t0 = time.perf_counter()
  kernels.sgd_mf_host((m, n), indptr, indices, vals, hu, hm)
  host_ms = [(time.perf_counter() - t0) * 1e3]
  assert ud.numpy().tobytes() == hu.tobytes() and md.numpy().tobytes() == hm.tobytes(), 'device and host loop differ'

  variants = []
  for w in WIDES:
    if w > 1 and w != WIDES[-1] and not ((widths >= w).any() and (widths < w).any()) and w != _hip.SP_MF_WIDE:
      continue                                           # (cuts nothing another w does not cut)
    p = resegment(plan, w)
    variants.append(('wide_%d' % w, p, be.from_numpy(p), len(kernels.sgd_mf_plan_parts(p)['segments'])))
  for _, p, pd, _ in variants:
    kernels.sgd_mf((m, n), dvals, pd, p, ud, md)
  D.synchronize()
  ms = {label: [] for label, _, _, _ in variants}
  for _ in range(reps):
    for label, p, pd, _ in variants:
      e0, e1 = kernels.Event(), kernels.Event()
      e0.record()
      kernels.sgd_mf((m, n), dvals, pd, p, ud, md)
      e1.record()
      e1.synchronize()
      ms[label].append(e0.elapsed_ms(e1))
  for _ in range(2 if nnz > 100000 else reps):
    t0 = time.perf_counter()
    kernels.sgd_mf_host((m, n), indptr, indices, vals, hu, hm)
    host_ms.append((time.perf_counter() - t0) * 1e3)
  launches = {label: k for label, _, _, k in variants}
  launches['host'] = 0
  ms['host'] = host_ms
  for label, v in ms.items():
    med = float(np.median(v))
    emit(dict(base, variant=label, ms=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), reps=len(v),
              launches=launches[label], ratings_per_s=float('%.4g' % (nnz / med * 1e3)),
              ns_per_rating=float('%.4g' % (med * 1e6 / nnz)), us_per_level=float('%.4g' % (med * 1e3 / max(levels, 1)))))
  best = min((l for l in ms if l != 'host'), key=lambda l: np.median(ms[l]))
  emit(dict(base, variant='summary', best=best, built_in='wide_%d' % _hip.SP_MF_WIDE,
            host_over_built_in=round(float(np.median(ms['host']) / np.median(ms['wide_%d' % _hip.SP_MF_WIDE])), 2),
            host_over_best=round(float(np.median(ms['host']) / np.median(ms[best])), 2)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=None)
  ap.add_argument('--tiles', default='golden,narrow,bench')
  args = ap.parse_args()
  import spartan_amd as sp
  be = sp.initialize('hip', num_workers=1).backend
  rows = []

  def emit(row):
    print(json.dumps(row), flush=True)
    rows.append(row)
    if args.out:
      with open(args.out, 'w') as fh:
        json.dump(rows, fh, indent=1)
  try:
    for name in args.tiles.split(','):
      for f in TILES[name][3]:
        for dtype in ('float32', 'float64'):
          run(be, name, f, dtype, args.reps, emit)
  finally:
    sp.shutdown()


if __name__ == '__main__':
  main()
