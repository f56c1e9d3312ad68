"""Records tests/golden/fuzzy_w4.npz: the reference's own fuzzy k-means tile bodies (spartan/examples/fuzzy_kmeans.py,
kmeans_map2_dist_mapper and kmeans_map2_center_mapper) on the small input of tests/test_fuzzy_example.py, with the
helpers of make_golden.py (the reference tree is copied to a scratch directory, transliterated to Python 3 there and
run in process; only the arrays are kept).

  python tests/golden/make_golden_fuzzy.py

  points            96 x 7 float64, uniform in [0, 1)
  centers0          5 x 7 float64 starting centres
  m{2,1.5}_{fuzzy,centers,labels}{1,2}
                    the two mappers chained by this script for two iterations from centers0: fuzzy = dist mapper,
                    labels = argmax(fuzzy, axis=1), centers = center mapper / sum(fuzzy ** m, axis=0)[:, None]
  m{2,1.5}_labels_w4
                    the reference's whole fuzzy_kmeans(points, k=5, num_iter=2, m, centers0) at 4 workers, if the
                    transliterated reference evaluates it; otherwise the script prints what stopped it

The script asserts that in every row of every recorded membership matrix the two largest entries differ by at least
1e-3 relative (a float32 run must then find the same labels); the seed of the input was picked so that they do.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import test_fuzzy_example as case  # noqa: E402

WORKERS = 4


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  mg.install_stubs()
  sp = mg.import_reference()
  from spartan.array import extent
  from spartan.examples import fuzzy_kmeans as ref
  x, c0 = np.array(case.points()), np.array(case.start_centers())
  out = dict(points=x, centers0=c0)
  ex = extent.create((0, 0), x.shape, x.shape)
  for m in case.MS:
    tag = 'm%g_' % m
    c = c0
    for it in ('1', '2'):
      (_, fuzzy), = list(ref.kmeans_map2_dist_mapper([ex], [x], centers=c, m=m))
      fuzzy = np.asarray(fuzzy, np.float64)
      (_, sums), = list(ref.kmeans_map2_center_mapper([ex], [x, fuzzy], centers=c, m=m))
      c = np.asarray(sums, np.float64) / np.sum(fuzzy ** m, axis=0)[:, np.newaxis]
      top = np.sort(fuzzy, axis=1)
      gap = float(((top[:, -1] - top[:, -2]) / top[:, -1]).min())
      print('fuzzy_w4.npz: m = %g, iteration %s: the two largest memberships of a row differ by at least %.3g relative'
            % (m, it, gap))
      assert gap >= 1e-3
      out.update({tag + 'fuzzy' + it: fuzzy, tag + 'centers' + it: c, tag + 'labels' + it: np.argmax(fuzzy, axis=1).astype(np.int64)})
    try:
      mg.start_cluster(sp, WORKERS)
      from spartan.config import FLAGS
      FLAGS.num_workers = WORKERS
      labels = ref.fuzzy_kmeans(sp.from_numpy(x.copy()), k=c0.shape[0], num_iter=2, m=m, centers=sp.from_numpy(c0.copy()))
      labels = np.asarray(labels.glom(), np.int64)
      print('fuzzy_w4.npz: m = %g: fuzzy_kmeans() evaluated at %d workers; %d of %d labels differ from the chained labels2'
            % (m, WORKERS, int(np.count_nonzero(labels != out[tag + 'labels2'])), labels.size))
      out[tag + 'labels_w4'] = labels
    except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
      print("fuzzy_w4.npz: the reference's fuzzy_kmeans() (m = %g) did not evaluate:" % m, type(e).__name__, str(e)[:400])
  path = os.path.join(HERE, 'fuzzy_w4.npz')
  np.savez_compressed(path, **out)
  print('fuzzy_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out))


if __name__ == '__main__':
  main()
