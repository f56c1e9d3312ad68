"""Times the item recommender's fused cosine top-k kernel (sp_item_topk) against the reference's N x N similarity table
built on the GEMM, map and sort kernels of the same build in the same run, and against the vector pipe's issue rate.

  python tools/bench_cf.py [--reps 5] [--out profiles/cf_rates.json]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Steps (users x items, dtype, k):
  8000 x 800 float64 k = 10, density 0.1: the reference's own benchmark (tests/test_item_recommender.py); here also one
      whole ItemBasedRecommender(...).precompute() per method on the csr sparse_rand table, by the host clock
  65536 x 8192 and 65536 x 16384, float32 and float64, k = 10 and 128: enough to load the device
  512 x 262144 float32 k = 10: 'table' is not run -- its N x N array alone is 256 GiB, which does not fit beside the
      operands in the device's memory; the step says so in its summary line
The large tables are drawn on the device (standard normal by the backend's generator); the 8000 x 800 one is the
sparse_rand table made dense.  Per step the variants are warmed up once each and then timed ALTERNATELY, `reps` rounds
(HIP events on the library's stream); every figure is the median (min and max beside it).  Variants:
  fused   backend.item_topk(table, norms, table, norms, k): one call, the whole table as one band
  table   ItemBasedRecommender(method='table')._table(): dot(r^T, r) on the MFMA GEMM, the outer product of norms,
          the division and nan_to_num on the map kernels, argsort and sort of the N x N table, the first k columns
          brought to the host.  The events also see the host building and lowering the expressions.
One JSON line per variant:
  ms                  one call
  pair_users_per_s    items * items * users / ms  (fused and table)
  valu_per_pair_user  (fused) vector instructions per pair and user in the kernel's inner loop, read from the ISA of
                      this build's flags (hipcc -S on csrc/cf.hip, the loop over a full chunk, 4 users unrolled: 78
                      vector instructions per 64 pair-users in float32 -- 32 v_pk_mul_f32 and 32 v_pk_add_f32, two pairs
                      each -- and 146 in float64 -- 64 v_mul_f64 and 64 v_add_f64)
  of_valu_issue       (fused) pair_users_per_s * valu_per_pair_user over the chip's vector issue rate, taken as 256 CUs
                      x 4 SIMDs x one wave64 instruction per 2 cycles at 2.4 GHz = 1228.8 G wave-instructions/s x 64
                      lanes.  A float64 instruction takes more than 2 cycles, so 1.0 is not reachable in float64; the
                      clock under load is below 2.4 GHz as well.
and one line `summary` per step with fused_over_table (ms over ms) where table ran.
Before timing, 8 targets against 512 sources of the step are checked against the oracle and the derived bound of the
test-suite, and (where table ran) the two variants' index sets are compared."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (users, items, dtype, k, density or None, run table)
STEPS = ((8000, 800, 'float64', 10, 0.1, True),) + tuple(
    (65536, items, name, k, None, True) for items in (8192, 16384) for name in ('float32', 'float64') for k in (10, 128)
) + ((512, 262144, 'float32', 10, None, False),)
STEP_SECONDS = 420
VALU_PER_PAIR_USER = {'float32': 78 / 64.0, 'float64': 146 / 64.0}
WAVE_INSTRUCTIONS_PER_S = 256 * 4 * 2.4e9 / 2


def _key(step):
  return '%d:%d:%s:%d' % step[:4]


def _check(be, table, norms, k):
  from tests import cf_cases as cc
  users, items = table.shape
  t0, s0 = items // 2, max(0, items // 3 - 256)
  m, ns = min(8, items - t0), min(512, items - s0)
  t, tn = table[:, t0:t0 + m], norms[t0:t0 + m]
  s, sn = table[:, s0:s0 + ns], norms[s0:s0 + ns]
  sim, idx = be.item_topk(t, tn, s, sn, k, index_offset=s0)
  exact, bound = cc.oracle(t.numpy(), tn.numpy(), s.numpy(), sn.numpy())
  worst, _, _ = cc.check_topk(sim.numpy(), idx.numpy(), exact, bound, k, index_offset=s0, label='bench %d x %d' % (users, items))
  assert worst <= 1.0, worst
  return worst


def step(spec, reps):
  import spartan_amd as sp
  from spartan_amd import devarray as D, expr, kernels
  from spartan_amd.array import extent
  from spartan_amd.examples.cf import ItemBasedRecommender
  users, items, name, k, density, with_table = spec
  dtype = np.dtype(name)
  be = sp.initialize('hip', num_workers=1).backend
  sparse = None
  if density is not None:
    sparse = expr.evaluate(sp.sparse_rand((users, items), dtype=dtype, density=density, format='csr'))
    dense = np.asarray(sparse.glom().todense(), dtype)
    array = expr.evaluate(expr.from_numpy(dense, tile_hint=(users, items)))
  else:
    expr.set_random_seed(20261020)
    array = expr.evaluate(expr.astype(expr.randn(users, items, tile_hint=(users, items)), dtype))
  table = array.fetch(extent.from_shape(array.shape))
  model = ItemBasedRecommender(array, k, method='table')
  norms = expr.evaluate(expr.astype(model._get_norm_of_each_item(model.rating_table), dtype))
  norms = norms.fetch(extent.from_shape(norms.shape))
  share = _check(be, table, norms, k)

  def fused():
    return be.item_topk(table, norms, table, norms, k)

  def as_table():
    out = model._table()
    del model.similarity_table
    return out

  variants = [('fused', fused)]
  if with_table:
    variants.append(('table', as_table))
  first = {label: fn() for label, fn in variants}
  D.synchronize()
  agree = None
  if with_table:
    ours, theirs = first['fused'][1].numpy(), first['table'][1]
    agree = float(np.mean([len(set(a.tolist()) & set(b.tolist())) / float(k) for a, b in zip(ours, theirs)]))
  del first
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
  if sparse is not None:
    for method in ('fused', 'table'):
      ItemBasedRecommender(sparse, k, method=method).precompute()           # (warm-up)
      D.synchronize()
      ms['precompute_' + method] = []
      for _ in range(reps):
        t0 = time.perf_counter()
        ItemBasedRecommender(sparse, k, method=method).precompute()
        D.synchronize()
        ms['precompute_' + method].append((time.perf_counter() - t0) * 1e3)
  med = {label: float(np.median(v)) for label, v in ms.items()}
  for label in ms:
    row = dict(kernel='item_topk', variant=label, dtype=name, users=users, items=items, k=k, ms=round(med[label], 4),
               ms_min=round(min(ms[label]), 4), ms_max=round(max(ms[label]), 4), reps=reps)
    if label in ('fused', 'table'):
      row['pair_users_per_s'] = float('%.4g' % (float(items) * items * users / med[label] * 1e3))
    if label == 'fused':
      row['valu_per_pair_user'] = round(VALU_PER_PAIR_USER[name], 4)
      row['of_valu_issue'] = round(row['pair_users_per_s'] * VALU_PER_PAIR_USER[name] / (WAVE_INSTRUCTIONS_PER_S * 64), 4)
      row['share_of_bound'] = float('%.3g' % share)
    print(json.dumps(row), flush=True)
  summary = dict(kernel='item_topk', variant='summary', dtype=name, users=users, items=items, k=k)
  if 'table' in med:
    summary['fused_over_table'] = round(med['fused'] / med['table'], 4)
    summary['index_sets_shared'] = round(agree, 6)
  else:
    summary['table_skipped'] = ('the N x N similarity table alone is %.0f GiB and does not fit beside the operands'
                                % (float(items) * items * dtype.itemsize / 2 ** 30))
  if 'precompute_fused' in med:
    summary['precompute_fused_over_precompute_table'] = round(med['precompute_fused'] / med['precompute_table'], 4)
  print(json.dumps(summary), flush=True)
  sp.shutdown()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=None)
  ap.add_argument('--only', default=None, help='run only the steps whose key users:items:dtype:k contains this text')
  ap.add_argument('--step', default=None, help='(internal) run one step in this process: users:items:dtype:k')
  args = ap.parse_args()
  by_key = {_key(s): s for s in STEPS}
  if args.step:
    if args.step not in by_key:
      raise SystemExit('unknown step %r' % args.step)
    step(by_key[args.step], args.reps)
    return
  rows = []
  for spec in STEPS:
    if args.only and args.only not in _key(spec):
      continue
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', _key(spec),
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
      raise SystemExit('bench_cf: step %s ended with status %d; nothing further is started' % (_key(spec), proc.returncode))


if __name__ == '__main__':
  main()
