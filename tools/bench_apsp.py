"""Times kernels.apsp (sp_apsp: blocked Floyd-Warshall) with HIP events on the library's stream, beside the host route the
reference's Isomap takes for the same step -- a Dijkstra per source over the sparse neighbour graph, here
scipy.sparse.csgraph.shortest_path(method='D') -- and one whole Isomap.fit split by step.

  python tools/bench_apsp.py [--n 1024,4096,8192,16384] [--dtype float32,float64] [--k 10] [--reps 5]
                             [--host-limit 60] [--isomap 1024] [--out profiles/apsp_rates.json]

The graph: every vertex lists k vertices drawn at random with weights uniform in [0.5, 2), made undirected by
backend.graph_from_knn.  Every figure is the median of `reps` runs after one warm-up run; the matrix is copied into the
work buffer outside the events.  One JSON line per case:
  ms                      one kernels.apsp call
  gcand_per_s             n^3 / ms: candidates (one add, one min each) per second, in units of 1e9
  launches                1 + 3 ceil(n / 64) kernel launches of that call (2 when n <= 64)
  host_s, gpu_over_host   scipy's Dijkstra on the same graph (float64, one core) and host_s / (ms / 1e3); the host leg
                          goes up in n and stops before the size whose predicted time (4.5 x the one before) passes
                          --host-limit seconds
  checked                 at the smallest n the device result is held to the oracle and the bound of tests/apsp_cases.py
The --isomap case runs the driver's steps one at a time on one worker, the device drained after each, on the host clock."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import spartan_amd as sp  # noqa: E402
from spartan_amd import devarray as D, kernels  # noqa: E402


def _lists(n, k, dtype, seed=20150712):
  rng = np.random.RandomState(seed)
  return rng.uniform(0.5, 2.0, size=(n, k)).astype(dtype), rng.randint(0, n, size=(n, k)).astype(np.int64)


def _time_apsp(be, w, reps):
  work, info = be.empty(tuple(w.shape), w.dtype), be.empty((1,), np.int32)
  box = tuple(slice(0, n) for n in w.shape)
  out = []
  for r in range(reps + 1):
    be.paste(work, box, w)
    e0, e1 = kernels.Event(), kernels.Event()
    e0.record()
    kernels.apsp(work, info)
    e1.record()
    e1.synchronize()
    if r:
      out.append(e0.elapsed_ms(e1))
  assert int(info.numpy()[0]) == 0
  return float(np.median(out)), float(min(out)), float(max(out)), work


def _host_dijkstra(w_host):
  from scipy.sparse import csr_matrix
  from scipy.sparse.csgraph import shortest_path
  n = w_host.shape[0]
  edge = np.isfinite(w_host) & ~np.eye(n, dtype=bool)
  i, j = np.nonzero(edge)
  g = csr_matrix((w_host[edge].astype(np.float64), (i, j)), shape=(n, n))
  t = time.perf_counter()
  out = shortest_path(g, method='D', directed=False)
  return time.perf_counter() - t, out


def _isomap_steps(n, dtype, k):
  from spartan_amd.examples import _dense
  from spartan_amd.examples.sklearn.manifold import Isomap, _graph
  rng = np.random.RandomState(20150713)
  t = 3 * np.pi * (rng.rand(n) - 0.5)
  x = np.stack([np.sin(t), 2.0 * rng.rand(n), np.sign(t) * (np.cos(t) - 1)], axis=1).astype(dtype)
  be = sp.initialize('hip', num_workers=1).backend
  steps = {}

  def timed(name, fn):
    D.synchronize()
    t0 = time.perf_counter()
    out = fn()
    D.synchronize()
    steps[name] = round((time.perf_counter() - t0) * 1e3, 3)
    return out

  iso = Isomap(n_neighbors=k)
  for attempt in ('warm', 'timed'):
    dist, ind = timed('neighbours_ms', lambda: iso._neighbour_lists(sp.from_numpy(x)))
    graph = timed('graph_ms', lambda: _graph.graph_from_knn(dist, ind))
    geo = timed('apsp_ms', lambda: _graph.apsp(graph))

    def centre():
      z = np.where(geo < np.inf, geo, geo.dtype.type(0))
      g = z * z * -0.5
      return g - g.mean(axis=1, keepdims=True) - g.mean(axis=0, keepdims=True) + g.mean()
    G = timed('centre_ms', centre)
    timed('syev_ms', lambda: _dense.syev(G))
    sweeps = be.syev_sweeps
    timed('fit_ms', lambda: Isomap(n_neighbors=k).fit(sp.from_numpy(x)))
  sp.shutdown()
  return dict(kernel='isomap_fit', dtype=np.dtype(dtype).name, n=n, n_neighbors=k, syev_sweeps=sweeps, **steps)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', default='1024,4096,8192,16384')
  ap.add_argument('--dtype', default='float32,float64')
  ap.add_argument('--k', type=int, default=10)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--host-limit', type=float, default=60.0)
  ap.add_argument('--isomap', type=int, default=1024)
  ap.add_argument('--out', default=None)
  args = ap.parse_args()
  rows = []

  def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)
    if args.out:
      with open(args.out, 'w') as f:
        json.dump(rows, f, indent=1)

  sizes = sorted(int(v) for v in args.n.split(',') if v)
  be = sp.initialize('hip', num_workers=1).backend
  host = {}
  last = None
  for n in sizes:                      # the host leg first: it does not depend on the dtype under test
    if args.host_limit <= 0 or (last is not None and last * 4.5 > args.host_limit):
      break
    dist, idx = _lists(n, args.k, np.float64)
    w = be.graph_from_knn(be.from_numpy(dist), be.from_numpy(idx)).numpy()
    last, _ = _host_dijkstra(w)
    host[n] = last
  for name in (v for v in args.dtype.split(',') if v):
    dtype = np.dtype(name)
    for n in sizes:
      try:
        dist, idx = _lists(n, args.k, dtype)
        w = be.graph_from_knn(be.from_numpy(dist), be.from_numpy(idx))
        ms, lo, hi, result = _time_apsp(be, w, args.reps)
      except Exception as e:   # noqa: BLE001  (a size that does not fit in memory is reported and the run goes on)
        emit(dict(kernel='apsp', dtype=dtype.name, n=n, skipped='%s: %s' % (type(e).__name__, str(e)[:200])))
        continue
      nb = -(-n // 64)
      row = dict(kernel='apsp', dtype=dtype.name, n=n, k=args.k, ms=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                 gcand_per_s=round(float(n) ** 3 / ms / 1e6, 2), launches=2 if nb == 1 else 1 + 3 * nb)
      if n in host:
        row.update(host_s=round(host[n], 4), gpu_over_host=round(host[n] / (ms / 1e3), 2))
      if n == sizes[0] and n in host:
        from tests import apsp_cases
        apsp_cases.check_real(result.numpy(), w.numpy(), label='bench')
        row.update(checked=True)
      emit(row)
      del w, result
  sp.shutdown()
  if args.isomap > 0:
    emit(_isomap_steps(args.isomap, np.float32, args.k))


if __name__ == '__main__':
  main()
