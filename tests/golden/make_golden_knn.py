"""Records tests/golden/knn_w4.npz: the reference's own NearestNeighbors (spartan/examples/sklearn/neighbors/
unsupervised.py) run at 4 workers on the 37 x 1031 x 33 float64 input of tests/knn_cases.py, with the helpers of
make_golden.py (the reference tree is copied to a scratch directory, transliterated to Python 3 there and run in
process; only the arrays are kept).

  python tests/golden/make_golden_knn.py

  q, x          the input
  dist, ind     NearestNeighbors(5, 'kd_tree'): its per-tile scheme (scikit-learn's kd-tree on every tile of X, the
                candidates sorted on the master); needs foreach_tile, fetch and glom only
  brute_dist, brute_ind   its 'brute' expression path with n_neighbors passed to kneighbors (the raw argument is what
                its column cut uses), if the transliterated reference evaluates it; otherwise the script says what
                stopped it and the file holds the first two only

Before saving, the script asserts that the recorded distances of each row are more than 4 gamma apart (relative, gamma
of tests/knn_cases.py for d = 33 in float64), so that the recorded indices are the only right answer."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import knn_cases  # noqa: E402

NQ, NP, D, K = 37, 1031, 33, 5


def prepare_neighbors():
  """lib2to3 over the neighbours driver (prepare_examples stops at sklearn/cluster)."""
  d = os.path.join(mg.SCRATCH, 'spartan', 'examples', 'sklearn', 'neighbors')
  files = [os.path.join(d, f) for f in os.listdir(d) if f.endswith('.py')]
  subprocess.check_call([sys.executable, '-m', 'lib2to3', '-w', '-n', '-x', 'map', '-x', 'filter', '-x', 'reduce',
                         '-x', 'zip', '-x', 'import'] + files, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  prepare_neighbors()
  mg.install_stubs()
  sp = mg.import_reference()
  from spartan.config import FLAGS
  from spartan.examples.sklearn.neighbors.unsupervised import NearestNeighbors
  q, x = knn_cases.real_case(NQ, NP, D, np.float64)
  out = dict(q=q, x=x)
  mg.start_cluster(sp, 4)
  FLAGS.num_workers = 4
  # (the per-tile path calls foreach_tile on what fit() was given: an evaluated array, not an expression.  X in four
  # tiles of 258, 258, 258 and 257 rows: the reference's default cut of 1031 rows over 4 workers ends in a fifth tile of
  # 3 rows, and scikit-learn refuses to look for 5 neighbours among 3 points)
  fitted = sp.from_numpy(x, tile_hint=(258, D)).evaluate()
  dist, ind = NearestNeighbors(K, 'kd_tree').fit(fitted).kneighbors(sp.from_numpy(q))
  dist, ind = np.asarray(dist, np.float64), np.asarray(ind, np.int64)
  assert dist.shape == (NQ, K) and ind.shape == (NQ, K)
  g = knn_cases.gamma(D, np.float64)
  gaps = np.diff(dist, axis=1) / dist[:, 1:]
  print('knn_w4.npz: smallest relative gap between the recorded distances of a row: %.3g (4 gamma = %.3g)'
        % (gaps.min(), 4 * g))
  assert gaps.min() > 4 * g
  want_d, want_i = knn_cases.oracle(q, x, K)
  assert np.array_equal(ind, want_i), 'the reference and the oracle of tests/knn_cases.py disagree'
  out.update(dist=dist, ind=ind)
  try:
    mg.start_cluster(sp, 4)
    FLAGS.num_workers = 4
    bd, bi = NearestNeighbors(K, 'brute').fit(sp.from_numpy(x)).kneighbors(sp.from_numpy(q), n_neighbors=K)
    bd, bi = np.asarray(bd, np.float64), np.asarray(bi)
    print("knn_w4.npz: 'brute' evaluated: dist", bd.shape, 'ind', bi.dtype, bi.shape,
          'same indices as kd_tree:', bool(np.array_equal(bi.astype(np.int64), ind)))
    out.update(brute_dist=bd, brute_ind=bi)
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    print("knn_w4.npz: the reference's 'brute' path did not evaluate:", type(e).__name__, str(e)[:400])
  np.savez_compressed(os.path.join(HERE, 'knn_w4.npz'), **out)
  print('knn_w4.npz:', os.path.getsize(os.path.join(HERE, 'knn_w4.npz')), 'bytes')


if __name__ == '__main__':
  main()
