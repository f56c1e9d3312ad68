"""Times backend.als_solve (sp_als_solve: one ALS half-step) with HIP events on the library's stream.

  python tools/bench_als.py [--reps 5] [--out profiles/als_rates.json] [--skip-cpu]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Steps:
  reference   the reference benchmark's shape (its tests/test_als.py: 320 x 12800 ratings, f = 20, implicit feedback,
              ratings randint(0, 5)): the U half-step on the 320 x 12800 matrix and the M half-step on its transpose,
              float64 (the reference's precision) and float32
  square      12800 x 12800 ratings, both modes, f in {8, 20, 32, 64}, one step per dtype
  cpu         the reference's formulation of the two `reference` half-steps -- its mapper loop over rows around
              scipy.linalg.lstsq, restated here (not imported) -- on one core of this machine, float64
Ratings and factors are drawn on the host from a seed.  The ratings of the small shape are rotated through copies
(512 MiB in all) so that no call finds them in the 256 MiB cache from the call before; the square matrix is larger than
the cache by itself.  Every figure is the median of `reps` runs after a warm-up run per copy; one JSON line per case:
  ms                 one backend.als_solve call (events around it: the pre-pass of implicit mode, the row kernel and the
                     info hand-off; the output tile's allocation is inside, as in the driver)
  useful_tfma        nnz f (f + 1) / 2 fused multiply-adds (the lower triangle of every rated item's y y^T) / ms
  of_vector_peak     2 useful_tfma / the vector peak of the dtype (157.3 TFLOP/s fp32, 78.6 fp64: an FMA counts two)
  r_gbps, of_copy    bytes of R read once / ms, and that over the 6.29 TB/s a float4 device copy measures on this chip
  limit              the larger of the two shares names the limit the kernel sits nearer to
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_VECTOR_TFLOPS = {'float32': 157.3, 'float64': 78.6}
COPY_TBPS = 6.29
LA, ALPHA, SEED = 0.065, 40.0, 20150715
STEP_SECONDS = {'reference': 240, 'square': 420, 'cpu': 600}


def _inputs(m, n, f, dtype):
  rng = np.random.RandomState(SEED)
  return rng.randint(0, 5, size=(m, n)).astype(dtype), rng.rand(n, f).astype(dtype)


def _time(be, copies, y, implicit, reps):
  from spartan_amd import devarray as D, kernels
  for r in copies:
    be.als_solve(r, y, LA, ALPHA, implicit=implicit)
  D.synchronize()
  out = []
  for i in range(reps):
    r = copies[i % len(copies)]
    e0, e1 = kernels.Event(), kernels.Event()
    e0.record()
    be.als_solve(r, y, LA, ALPHA, implicit=implicit)
    e1.record()
    e1.synchronize()
    out.append(e0.elapsed_ms(e1))
  return float(np.median(out)), float(min(out)), float(max(out))


def _row(kind, m, n, f, dtype, implicit, nnz, ms, lo, hi, copies):
  tfma = nnz * f * (f + 1) / 2.0 / ms / 1e9
  of_peak = 2.0 * tfma / PEAK_VECTOR_TFLOPS[dtype.name]
  gbps = m * n * dtype.itemsize / ms / 1e6
  of_copy = gbps / 1e3 / COPY_TBPS
  return dict(kernel='als_solve', step=kind, dtype=dtype.name, m=m, n=n, f=f, mode='implicit' if implicit else 'explicit',
              nnz=int(nnz), ms=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), useful_tfma=round(tfma, 3),
              of_vector_peak=round(of_peak, 4), r_gbps=round(gbps, 1), of_copy=round(of_copy, 4),
              limit='vector pipe' if of_peak >= of_copy else 'reading R', copies_of_r=copies)


def _check(be, r, y, implicit, got):
  """The first rows of what was timed against the oracle and the derived bound of the test-suite."""
  from tests import als_cases
  rows = min(4, r.shape[0])
  want, bound, _ = als_cases.oracle(r[:rows], y, LA, ALPHA, implicit)
  als_cases.check(got[:rows], want, bound, 'bench rows')


def step_reference(reps):
  import spartan_amd as sp
  be = sp.initialize('hip', num_workers=1).backend
  for dtype in (np.dtype(np.float64), np.dtype(np.float32)):
    for m, n in ((320, 12800), (12800, 320)):
      r, y = _inputs(m, n, 20, dtype)
      n_copies = max(1, min(32, -(-(512 << 20) // r.nbytes)))
      copies = [be.from_numpy(np.roll(r, c, axis=0)) for c in range(n_copies)]
      yt = be.from_numpy(y)
      _check(be, r, y, True, be.als_solve(copies[0], yt, LA, ALPHA, implicit=True).numpy())
      ms, lo, hi = _time(be, copies, yt, True, reps)
      print(json.dumps(_row('reference', m, n, 20, dtype, True, np.count_nonzero(r), ms, lo, hi, n_copies)), flush=True)
      del copies
  sp.shutdown()


def step_square(reps, dtype):
  import spartan_amd as sp
  dtype = np.dtype(dtype)
  be = sp.initialize('hip', num_workers=1).backend
  m = n = 12800
  r, _ = _inputs(m, n, 1, dtype)
  rt = be.from_numpy(r)
  nnz = np.count_nonzero(r)
  for f in (8, 20, 32, 64):
    y = np.random.RandomState(SEED + f).rand(n, f).astype(dtype)
    yt = be.from_numpy(y)
    for implicit in (False, True):
      if f == 20:
        _check(be, r, y, implicit, be.als_solve(rt, yt, LA, ALPHA, implicit=implicit).numpy())
      ms, lo, hi = _time(be, [rt], yt, implicit, reps)
      print(json.dumps(_row('square', m, n, f, dtype, implicit, nnz, ms, lo, hi, 1)), flush=True)
  sp.shutdown()


def _reference_half_step(r, y, la, alpha):
  """spartan/examples/als.py:27-46, 61-69 restated: the implicit-feedback mapper, row by row."""
  from scipy.linalg import lstsq
  yt = y.T
  yty = np.dot(yt, y)
  out = np.zeros((r.shape[0], y.shape[1]))
  for i in range(r.shape[0]):
    cu = r[i].reshape((r.shape[1], 1)) * alpha + 1
    a = np.dot(yt, y * (cu - 1)) + np.eye(y.shape[1]) * la
    b = (y * cu)[r[i] > 0].sum(axis=0)
    out[i] = lstsq(yty + a, b)[0]
  return out


def step_cpu():
  try:
    from threadpoolctl import threadpool_limits
    limit = threadpool_limits(limits=1)
  except ImportError:
    limit = None
  for m, n in ((320, 12800), (12800, 320)):
    r, y = _inputs(m, n, 20, np.dtype(np.float64))
    rows = min(m, 320)                       # (the tall half-step is timed on its first 320 rows and scaled)
    t = time.perf_counter()
    _reference_half_step(r[:rows], y, LA, ALPHA)
    s = (time.perf_counter() - t) * m / rows
    print(json.dumps(dict(kernel='reference_mapper_numpy_scipy', step='cpu', dtype='float64', m=m, n=n, f=20,
                          mode='implicit', seconds=round(s, 3), rows_timed=rows,
                          blas_threads=1 if (limit is not None or os.environ.get('OMP_NUM_THREADS') == '1') else 'unpinned')),
          flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=None)
  ap.add_argument('--skip-cpu', action='store_true')
  ap.add_argument('--step', default=None, help='(internal) run one step in this process')
  args = ap.parse_args()
  if args.step:
    if args.step == 'reference':
      step_reference(args.reps)
    elif args.step.startswith('square:'):
      step_square(args.reps, args.step.split(':')[1])
    elif args.step == 'cpu':
      step_cpu()
    else:
      raise SystemExit('unknown step %r' % args.step)
    return
  steps = ['reference', 'square:float32', 'square:float64'] + ([] if args.skip_cpu else ['cpu'])
  rows = []
  for step in steps:
    env = dict(os.environ)
    if step == 'cpu':
      env.update(OMP_NUM_THREADS='1', OPENBLAS_NUM_THREADS='1', MKL_NUM_THREADS='1')
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS[step.split(':')[0]]), sys.executable, os.path.abspath(__file__),
           '--step', step, '--reps', str(args.reps)]
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, universal_newlines=True)
    for line in proc.stdout.splitlines():
      print(line, flush=True)
      if line.startswith('{'):
        rows.append(json.loads(line))
    if args.out:
      with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)
    if proc.returncode != 0:
      raise SystemExit('bench_als: step %r ended with status %d; nothing further is started' % (step, proc.returncode))


if __name__ == '__main__':
  main()
