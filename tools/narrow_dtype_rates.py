"""Rates of the bandwidth-bound tile kernels on narrow element types, next to fp32 and to the library's own copy.

One process, one GPU: `x*x+x`, `sum(x)` and `argmax(x, 1)` over N elements (default 2^30, as [N / 4096, 4096]) of
float32, int32, float16, int16 and int8 (int32: the int64 arithmetic class on a 4-byte type, so that the class's own cost
shows apart from the narrow loads), and sp_stream_copy of the same byte counts.  Every case is warmed up, then timed
`--repeats` times between device events, the cases of one round interleaved so that drift hits them alike.  Writes
elements/s, bytes/s, the fraction of the copy rate and the run-to-run spread to profiles/narrow_dtypes_rates.json.
A run without a GPU fails: nothing here is a CPU number.

  python tools/narrow_dtype_rates.py [--log2n 30] [--repeats 7] [--warmup 2] [--out profiles/narrow_dtypes_rates.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spartan_amd import _hip, kernels  # noqa: E402
from spartan_amd import devarray as D  # noqa: E402

DTYPES = ('float32', 'int32', 'float16', 'int16', 'int8')


def _fill(dt, shape):
  """Small integers in every type: exact everywhere, and the float16 sum of a row stays far below 65504."""
  dt = np.dtype(dt)
  rows, cols = shape
  out = D.empty(shape, dt)
  block = np.random.RandomState(7).randint(-3, 4, size=(min(rows, 4096), cols)).astype(dt)
  d = D.from_numpy(block)
  for r in range(0, rows, block.shape[0]):
    n = min(block.shape[0], rows - r)
    kernels.slice_copy(out, r * cols, (cols, 1), d, 0, (cols, 1), (n, cols))
  return out


def _timed(fn):
  e0, e1 = kernels.Event(), kernels.Event()
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_ms(e1) * 1e-3


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--log2n', type=int, default=30)
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--out', default=os.path.join('profiles', 'narrow_dtypes_rates.json'))
  args = ap.parse_args()
  n = 1 << args.log2n
  cols = min(4096, n)
  shape = (n // cols, cols)
  cases = {}
  for name in DTYPES:
    dt = np.dtype(name)
    x = _fill(dt, shape)
    dst = D.empty(shape, dt)
    out_sum = x.sum().dtype.itemsize
    cases[(name, 'map x*x+x')] = (lambda x=x: x * x + x, 2 * n * dt.itemsize)
    cases[(name, 'sum(x)')] = (lambda x=x: x.sum(), n * dt.itemsize + out_sum)
    cases[(name, 'argmax(x, 1)')] = (lambda x=x: x.argmax(1), n * dt.itemsize + shape[0] * 8)
    cases[(name, 'copy')] = (lambda x=x, dst=dst: kernels.stream_copy(dst, x), 2 * n * dt.itemsize)
  times = {k: [] for k in cases}
  lib = _hip.lib()
  jit_usable = lib.sp_jit_configure(-1, -1) == 1
  for rnd in range(args.warmup + args.repeats):
    if rnd == args.warmup:
      # every program outside the prebuilt fp32 library was asked for in the warm-up rounds: from here on it runs on
      # its run-time specialised kernel, not on the interpreter
      lib.sp_jit_wait()
      jit_compiled = lib.sp_jit_compiled_count()
    for k, (fn, _) in cases.items():
      t = _timed(fn)
      if rnd >= args.warmup:
        times[k].append(t)
  jit_after = lib.sp_jit_compiled_count()
  D.synchronize()
  rows = []
  for (name, what), ts in times.items():
    med = float(np.median(ts))
    nbytes = cases[(name, what)][1]
    copy = float(np.median(times[(name, 'copy')]))
    copy_rate = cases[(name, 'copy')][1] / copy
    f32 = float(np.median(times[('float32', what)]))
    rows.append({'dtype': name, 'case': what, 'elements': n, 'bytes': nbytes, 'seconds_median': med,
                 'seconds_min': float(min(ts)), 'seconds_max': float(max(ts)),
                 'spread': (float(max(ts)) - float(min(ts))) / med, 'elements_per_s': n / med, 'bytes_per_s': nbytes / med,
                 'fraction_of_copy_rate': (nbytes / med) / copy_rate, 'time_over_float32': med / f32})
  result = {'source_sha': _hip.source_sha(), 'elements': n, 'shape': list(shape), 'repeats': args.repeats,
            'warmup': args.warmup,
            'tier': {'jit_usable': bool(jit_usable), 'kernels_specialised_before_timing': int(jit_compiled),
                     'kernels_specialised_during_timing': int(jit_after - jit_compiled),
                     'note': 'sp_jit_wait() after the warm-up rounds: timed programs outside the prebuilt fp32 library '
                             'run on run-time specialised kernels'},
            'timing': 'device events around each call, cases interleaved per round', 'rows': rows}
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, 'w') as fh:
    json.dump(result, fh, indent=1)
  for r in rows:
    print('%-8s %-13s %8.3f ms  %7.1f Gelem/s  %6.2f TB/s  %5.2f of copy  spread %4.1f%%  x%.2f of float32' %
          (r['dtype'], r['case'], r['seconds_median'] * 1e3, r['elements_per_s'] / 1e9, r['bytes_per_s'] / 1e12,
           r['fraction_of_copy_rate'], 100 * r['spread'], r['time_over_float32']))


if __name__ == '__main__':
  main()
