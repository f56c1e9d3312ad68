"""Times one LDA (CVB0) step on a tile of documents (sp_lda_step) with HIP events on the library's stream, the fused
kernel against the same step phrased with the kernels the library had before it, on the same build in the same run.

  python tools/bench_lda.py [--reps 5] [--out profiles/lda_rates.json]

The parent process never opens the GPU: every step is a child (this file with --step) under its own `timeout`, and the
first step that fails, faults or runs out of time ends the run.  Steps (float32, one inner iteration, alpha = eta = 0.1):
  test      160 terms x 200 documents, k = 16: the reference's own test shape per worker
  real16    41 807 terms x 21 578 documents, dense, k = 16: the shape the reference's driver names as its real input
  real128   the same at k = 128
Counts are drawn on the host from a seed (integers 0 .. 4, about half the entries 0), N uniform in [0, 1).  Per step
the variants are warmed up once each and then timed ALTERNATELY, `reps` rounds; every figure is the median (min and
max beside it).  Variants:
  fused        backend.lda_step(x, n, ...): delta and doc_topics; nothing of size V x D exists beside X
  fused_gamma  the same call with want_delta=False: lda_prep_kernel and lda_gamma_kernel only
  fused_prep   the call on no document, want_delta=False: lda_prep_kernel only
  baseline     A and B by map and reduce kernels, S = A^T B^T by the fp32 GEMM, W = X / S by a map kernel,
               c = B o (|W|^T |A|^T) and delta = A o (B^T W^T) by the GEMM again: three V x D temporaries (S, W, |W|)
One JSON line per variant:
  ms                 one call (events around it; the output tiles' allocation is inside, as in the driver)
  share              for the fused call, the share of each kernel: prep = fused_prep, gamma = fused_gamma - fused_prep,
                     delta (+ combine) = fused - fused_gamma
  vector_tflops      the vector-pipe operations sp_lda_step issues -- 2 V D KP per S tile sweep and per accumulation,
                     2 iters + 2 of them (2 iters without delta), KP = k rounded up to 16 .. 128 -- / ms
  of_vector_peak     that over the fp32 vector peak (157.3 TFLOP/s), which counts an FMA as two: the contract forbids
                     contraction, so a kernel of separate multiply / add tops out at one half
  vd_bytes           bytes of V x D temporaries the variant allocates and 'fused' does not
Before timing, the fused call and the baseline are checked against each other on the first 64 documents and (at most)
2048 terms inside twice the derived bound of the test-suite (each is inside it once against the exact result).
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_VECTOR_TFLOPS = 157.3
SHAPES = {'test': (160, 200, 16), 'real16': (41807, 21578, 16), 'real128': (41807, 21578, 128)}
ALPHA, ETA, ITERS, SEED = 0.1, 0.1, 1, 20151021
STEP_SECONDS = 540


def _inputs(v, d, k):
  rng = np.random.default_rng(SEED)
  x = rng.integers(0, 10, size=(v, d), dtype=np.int8)
  x[x >= 5] = 0
  return x.astype(np.float32), rng.random((k, v), dtype=np.float32)


def _fused(be, x, n):
  return be.lda_step(x, n, ALPHA, ETA, ITERS)


def _fused_gamma(be, x, n):
  return be.lda_step(x, n, ALPHA, ETA, ITERS, want_delta=False)


def _fused_prep(be, x, n):
  return be.lda_step(x[:, :0], n, ALPHA, ETA, ITERS, want_delta=False)


def _baseline(be, x, n):
  """The step with map, reduce and GEMM kernels only (float32); documents without a term are not treated."""
  from spartan_amd import devarray
  f = np.float32
  v, d = x.shape
  k = n.shape[0]
  den = np.abs(n).sum(axis=1) + f(ETA) * f(v)
  a = (n + f(ETA)) / den.reshape(k, 1)                      # [k, V]
  gamma = devarray.full((d, k), f(1) / f(k), f)
  for _ in range(ITERS):
    b = gamma + f(ALPHA)                                    # [D, k]
    s = a.T.dot(b.T)                                        # [V, D]
    w = x / s                                               # [V, D]
    c = b * np.abs(w).T.dot(np.abs(a).T)                    # [D, k]
    gamma = c / c.sum(axis=1).reshape(d, 1)
  return a * b.T.dot(w.T), gamma


VARIANTS = (('fused', _fused), ('fused_gamma', _fused_gamma), ('fused_prep', _fused_prep), ('baseline', _baseline))


def _check(be, x, n):
  from tests import lda_cases
  v, k = min(x.shape[0], 2048), n.shape[0]      # (the bound grows with V: at 41 807 terms it says nothing in float32)
  cols = np.ascontiguousarray(x[:v, :64])
  assert (cols != 0).any(axis=0).all()
  xt, nt = be.from_numpy(cols), be.from_numpy(np.ascontiguousarray(n[:, :v]))
  fused = [t.numpy() for t in _fused(be, xt, nt)]
  base = [t.numpy() for t in _baseline(be, xt, nt)]
  e = lda_cases.eps(v, 64, k, ITERS, np.float32)
  for name, got, want in zip(('delta', 'doc_topics'), fused, base):
    err = float(np.max(np.abs(got - want) / np.abs(want)))
    print('bench_lda: fused and baseline %s differ by %.3g relative (twice the bound: %.3g)' % (name, err, 2 * e[name]),
          flush=True)
    assert err <= 2 * e[name]


def step(name, reps):
  import spartan_amd as sp
  from spartan_amd import devarray as D, kernels
  v, d, k = SHAPES[name]
  be = sp.initialize('hip', num_workers=1).backend
  x, n = _inputs(v, d, k)
  _check(be, x, n)
  xt, nt = be.from_numpy(x), be.from_numpy(n)
  del x
  for _, fn in VARIANTS:
    fn(be, xt, nt)
  D.synchronize()
  ms = {label: [] for label, _ in VARIANTS}
  for _ in range(reps):
    for label, fn in VARIANTS:
      e0, e1 = kernels.Event(), kernels.Event()
      e0.record()
      out = fn(be, xt, nt)
      e1.record()
      e1.synchronize()
      ms[label].append(e0.elapsed_ms(e1))
      del out
  med = {label: float(np.median(ms[label])) for label, _ in VARIANTS}
  kp = 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128
  sweep = 2.0 * v * d * kp
  for label, _ in VARIANTS:
    t = med[label]
    row = dict(kernel='lda_step', variant=label, dtype='float32', V=v, D=d, k=k, iters=ITERS, ms=round(t, 3),
               ms_min=round(min(ms[label]), 3), ms_max=round(max(ms[label]), 3), reps=reps)
    if label in ('fused', 'fused_gamma'):
      ops = (2 * ITERS + (2 if label == 'fused' else 0)) * sweep
      row.update(vector_tflops=round(ops / t / 1e9, 2), of_vector_peak=round(ops / t / 1e9 / PEAK_VECTOR_TFLOPS, 4), vd_bytes=0)
    if label == 'fused':
      row['share'] = dict(prep=round(med['fused_prep'] / t, 4), gamma=round((med['fused_gamma'] - med['fused_prep']) / t, 4),
                          delta=round((t - med['fused_gamma']) / t, 4))
      row['baseline_over_fused'] = round(med['baseline'] / t, 3)
    if label == 'baseline':
      row['vd_bytes'] = 3 * v * d * 4
    print(json.dumps(row), flush=True)
  sp.shutdown()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--out', default=None)
  ap.add_argument('--steps', default='test,real16,real128')
  ap.add_argument('--step', default=None, help='(internal) run one step in this process')
  args = ap.parse_args()
  if args.step:
    if args.step not in SHAPES:
      raise SystemExit('unknown step %r' % args.step)
    step(args.step, args.reps)
    return
  rows = []
  for name in args.steps.split(','):
    cmd = ['timeout', '-k', '10', str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), '--step', name,
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
      raise SystemExit('bench_lda: step %r ended with status %d; nothing further is started' % (name, proc.returncode))


if __name__ == '__main__':
  main()
