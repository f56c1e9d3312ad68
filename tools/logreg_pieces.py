"""One gradient step of logistic regression as the reference spells it (logistic_regression.py:15-17, sgd.py:36-37),
timed on the configs[4] per-GPU tile (125 000 x 4096 fp32, operands generated in HBM), next to the 2 GiB stream copy
of the same run.  Only the public expression API: the same script runs on a commit without the one-pass rewrite of
this DAG (the step is then the dot launch + the fused map -> column-sum launch) and on one with it.

    python tools/logreg_pieces.py [--samples 9] [--steps 20]

Each sample is `steps` forced gradient steps between two HIP events, after warm-up (and after the run-time
specialisations the warm-up asked for have landed); samples alternate between the optimizer's default and
FLAGS['opt_rowdot_fusion'] = False, so both forms are measured in one process on one machine.  Prints one JSON line:
ms per step (median, min, max over the samples) and GB/s of 4.n.d bytes -- ONE pass over X, whatever the form reads --
for both, the same for the least-squares step (examples/lreg.py) as context, and the copy rate (bytes read + written)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spartan_amd as sp  # noqa: E402
from spartan_amd import _hip, devarray as D, kernels  # noqa: E402

optimize = importlib.import_module('spartan_amd.expr.optimize')


def uniform_tile(ex, seed):
  out = D.empty(ex.shape, np.float32)
  kernels.random_fill(out, 'uniform', seed + 1000003 * (ex.ul[0] if ex.ul else 0), 0)
  return out


def timed(fn, steps):
  e0, e1 = D.Event(), D.Event()
  e0.record()
  for _ in range(steps):
    fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_ms(e1) / steps


def summary(ms, nbytes):
  med = float(np.median(ms))
  return {'ms_per_step_median': round(med, 4), 'ms_per_step_min': round(min(ms), 4), 'ms_per_step_max': round(max(ms), 4),
          'spread_ms': round(max(ms) - min(ms), 4), 'GBps_of_one_pass': round(nbytes / med / 1e6, 1),
          'samples_ms': [round(v, 4) for v in ms]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--samples', type=int, default=9)
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--rows', type=int, default=125000)
  ap.add_argument('--cols', type=int, default=4096)
  a = ap.parse_args()
  ctx = sp.initialize('hip')
  N, Dm = a.rows, a.cols
  out = {'tile': '%dx%d fp32' % (N, Dm), 'samples': a.samples, 'steps_per_sample': a.steps}
  # the 2 GiB copy (bench.py's hbm section: 8192 x 65536 fp32 read and written)
  n = 8192 * 65536
  src, dst = D.empty((n,), np.float32), D.empty((n,), np.float32)
  kernels.random_fill(src, 'uniform', 7, 0)
  for _ in range(4):
    kernels.stream_copy(dst, src)
  D.synchronize()
  copy_ms = [timed(lambda: kernels.stream_copy(dst, src), 10) for _ in range(a.samples)]
  copy_gbps = 2 * 4.0 * n / float(np.median(copy_ms)) / 1e6
  out['stream_copy_2GiB'] = {'GBps_median': round(copy_gbps, 1), 'GBps_min': round(2 * 4.0 * n / max(copy_ms) / 1e6, 1),
                             'GBps_max': round(2 * 4.0 * n / min(copy_ms) / 1e6, 1)}
  del src, dst
  X = sp.Val(val=sp.from_tile_fn((N, Dm), np.float32, lambda ex: uniform_tile(ex, 11)).force())
  y = sp.Val(val=sp.from_tile_fn((N, 1), np.float32, lambda ex: uniform_tile(ex, 12)).force())
  w = ((np.random.RandomState(3).rand(Dm, 1) - 0.5) / 32).astype(np.float32)       # |x . w| stays small: no overflow

  def step():
    g = sp.exp(sp.dot(X, w))
    yp = g / (g + 1)
    return sp.sum(X * (yp - y), axis=0).optimized().force()

  def stated():
    optimize.FLAGS['opt_rowdot_fusion'] = False
    try:
      return step()
    finally:
      optimize.FLAGS['opt_rowdot_fusion'] = True
  g = sp.exp(sp.dot(X, w))
  out['default_form'] = type(sp.sum(X * (g / (g + 1) - y), axis=0).optimized()).__name__
  for fn in (step, stated):
    for _ in range(4):
      fn()
    _hip.lib().sp_jit_wait()
    for _ in range(2):
      fn()
  D.synchronize()
  a_val, b_val = step().glom(), stated().glom()
  out['finite'] = bool(np.isfinite(a_val).all())
  out['max_rel_diff_default_vs_stated'] = float(np.max(np.abs(a_val - b_val) / np.maximum(np.abs(b_val), 1e-30)))
  ms_default, ms_stated = [], []
  for _ in range(a.samples):                 # alternating: drift of the machine lands on both
    ms_default.append(timed(step, a.steps))
    ms_stated.append(timed(stated, a.steps))
  # context: the least-squares step of the same family on the same tile (examples/lreg.py), default form
  def lreg_step():
    return sp.sum(X * (sp.dot(X, w) - y), axis=0).optimized().force()
  for _ in range(4):
    lreg_step()
  _hip.lib().sp_jit_wait()
  lreg_step()
  D.synchronize()
  ms_lreg = [timed(lreg_step, a.steps) for _ in range(a.samples)]
  nbytes = 4.0 * N * Dm
  out['lreg_default'] = summary(ms_lreg, nbytes)
  out['default'] = summary(ms_default, nbytes)
  out['rewrite_off'] = summary(ms_stated, nbytes)
  out['default']['frac_of_measured_copy'] = round(out['default']['GBps_of_one_pass'] / copy_gbps, 3)
  out['rewrite_off']['frac_of_measured_copy'] = round(out['rewrite_off']['GBps_of_one_pass'] / copy_gbps, 3)
  print(json.dumps(out))
  sp.shutdown()


if __name__ == '__main__':
  main()
