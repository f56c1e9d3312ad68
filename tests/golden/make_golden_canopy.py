"""Records tests/golden/canopy_w4.npz: the reference's own canopy clustering (spartan/examples/canopy_clustering.py) on
the four inputs of tests/canopy_cases.py -- 160 rows around 6 blobs, float64 -- at 4 workers with cf = 1, with the
helpers of make_golden.py (the reference tree is copied to a scratch directory, transliterated to Python 3 there and run
in process; only the arrays are kept).  tests/canopy_cases.py lists what is recorded per setting.

  python tests/golden/make_golden_canopy.py

_canopy_mapper and _cluster_mapper are called directly, on a stand-in for the distributed array whose fetch() returns
the band; find_centers takes the bands' results in ascending order.  canopy_cluster itself is then run as a whole: if it
evaluates, its labels and the order in which it handed the bands to find_centers are recorded (whole_run = 1); if not,
the script prints what stopped it (whole_run = 0).

The script asserts that every distance the loops meet is at least 1e-6 (relative) away from t1 and t2, and that the two
largest pdfs of every row differ by at least 1e-9."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import canopy_cases as case  # noqa: E402


class _Band(object):
  """What the mappers ask of their array: fetch(ex) and shape."""

  def __init__(self, data):
    self.data, self.shape = data, data.shape

  def fetch(self, ex):
    return self.data[ex.ul[0]:ex.lr[0]]


def _gaps(points, t1, t2):
  """The smallest relative distance of a d2 the loop meets to t1 or t2 (every pair: a superset of what it meets)."""
  d2 = np.square(points[:, None, :] - points[None, :, :]).sum(axis=2)
  d2 = d2[~np.eye(len(points), dtype=bool)]
  return min(np.abs(d2 - t).min() / t for t in (t1, t2)) if len(points) > 1 else np.inf


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  mg.install_stubs()
  sp = mg.import_reference()
  from spartan.array import extent
  from spartan.examples import canopy_clustering as ref
  workers, cf = case.WORKERS, case.CF
  out = {}
  started = False
  for s in range(len(case.SETTINGS)):
    x, t1, t2 = case.golden_input(s)
    n, d = x.shape
    arr = _Band(x)
    blocks, gap = [], np.inf
    for b, (lo, hi) in enumerate(case.bands(n, workers)):
      ex = extent.create((lo, 0), (hi, d), (n, d))
      (_, got), = list(ref._canopy_mapper(arr, ex, t1, t2, cf))
      got = np.asarray(got, np.float64).reshape(-1, d)
      out['band_%d_%d' % (s, b)] = got
      blocks.append(got)
      gap = min(gap, _gaps(x[lo:hi], t1, t2))
    centers = np.asarray(ref.find_centers([[blk] for blk in blocks], t1, t2, cf), np.float64).reshape(-1, d)
    gap = min(gap, _gaps(np.concatenate(blocks), t1, t2))
    (_, labels), = list(ref._cluster_mapper(arr, extent.create((0, 0), (n, d), (n, d)), centers))
    pdf = np.sort(1.0 / (1 + np.square(x[:, None, :] - centers[None, :, :]).sum(axis=2)), axis=1)
    pdf_gap = (pdf[:, -1] - pdf[:, -2]).min() if centers.shape[0] > 1 else np.inf
    print('canopy_w4.npz setting %d: %s canopies per band, %d centres; nearest d2 to a threshold %.2g (relative), '
          'smallest gap of the two largest pdfs %.2g' % (s, [len(blk) for blk in blocks], len(centers), gap, pdf_gap))
    assert gap >= 1e-6 and pdf_gap >= 1e-9
    out.update({'centers_%d' % s: centers, 'labels_%d' % s: np.asarray(labels, np.int32)})

    whole, run_labels, order = 0, np.zeros(0, np.int32), np.zeros(0, np.int64)
    try:
      if not started:
        mg.start_cluster(sp, workers)
        from spartan.config import FLAGS
        FLAGS.num_workers = workers
        started = True
      seen = []
      real = ref.find_centers

      def watched(point_blocks, *a, **k):
        point_blocks = [list(bl) for bl in point_blocks]
        seen.extend(point_blocks)
        return real(point_blocks, *a, **k)

      ref.find_centers = watched
      try:
        pts = sp.from_numpy(np.array(x), tile_hint=(n // workers, d))
        run_labels = np.asarray(ref.canopy_cluster(pts, t1, t2, cf).glom(), np.int32).reshape(n)
      finally:
        ref.find_centers = real
      order = np.asarray([[b for b, blk in enumerate(blocks) if np.array_equal(np.asarray(bl[0]).reshape(-1, d), blk)][0]
                          for bl in seen], np.int64)
      whole = 1
      print('canopy_w4.npz setting %d: canopy_cluster() evaluated at %d workers; band order %s; labels equal to the '
            'ascending order\'s: %s' % (s, workers, order.tolist(), np.array_equal(run_labels, labels)))
    except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
      print("canopy_w4.npz setting %d: the reference's canopy_cluster() did not evaluate:" % s, type(e).__name__, str(e)[:400])
    out.update({'whole_run_%d' % s: np.asarray(whole, np.int64), 'run_labels_%d' % s: run_labels,
                'run_order_%d' % s: order})

  path = os.path.join(HERE, 'canopy_w4.npz')
  np.savez_compressed(path, **out)
  print('canopy_w4.npz:', os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
  main()
