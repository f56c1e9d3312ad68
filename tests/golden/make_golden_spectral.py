"""Records tests/golden/spectral_w4.npz: the reference's own spectral-clustering tile bodies
(spartan/examples/spectral_clustering.py, _row_similarity_mapper and _laplacian_mapper), its lanczos.solve and its whole
spectral_cluster on the small input of tests/spectral_cases.planted, with the helpers of make_golden.py (the reference
tree is copied to a scratch directory, transliterated to Python 3 there and run in process; only the arrays are kept).

  python tests/golden/make_golden_spectral.py

  points, truth     60 x 2 float64 points in three planted groups, truth = arange(60) % 3
  A_<metric>, D_<metric>, L_<metric>
                    for 'rbf', 'euclidean' and 'manhattan': the outputs of _row_similarity_mapper on the four bands of 15
                    rows stacked, their row sums, and the outputs of _laplacian_mapper on the same bands stacked
  lanczos_d, lanczos_s
                    lanczos.solve(L_rbf, L_rbf, 6, True) -- the reference's routine at 4 workers if the transliterated
                    reference evaluates it; otherwise the script prints what stopped it and records the project's own
                    host routine (examples/lanczos.ritz_pairs) with numpy.dot as the product; either way the two
                    are asserted to agree to 1e-9
  labels            k = 3, num_iter = 5: composed by this script from the recorded pieces (U = lanczos_s[:, :3], the
                    start U[argmax(U, axis=0)], Lloyd's iterations in NumPy)
  labels_w4         the reference's whole spectral_cluster(points, 3, 5) at 4 workers -- if the transliterated reference
                    evaluates it; otherwise the script prints what stopped it

The script asserts that the composed partition is the planted one and, when the whole run evaluates, that its
partition is the same."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from spartan_amd.examples.lanczos import ritz_pairs  # noqa: E402
from tests import spectral_cases as case  # noqa: E402

WORKERS = 4
BANDS = 4
K, NUM_ITER, RANK = 3, 5, 6


class Points(object):
  """What the reference's mappers ask of a distributed array: shape, tiles (the row bands) and fetch."""

  def __init__(self, data, extents):
    self.data, self.shape, self.tiles = data, data.shape, dict((ex, None) for ex in extents)

  def fetch(self, ex):
    return self.data[ex.to_slice()]


def lloyd(u, centres, num_iter):
  for _ in range(num_iter):
    labels = np.argmin(((u[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2), axis=1)
    centres = np.array([u[labels == j].mean(axis=0) if np.any(labels == j) else centres[j]
                        for j in range(centres.shape[0])])
  return labels


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  mg.install_stubs()
  sp = mg.import_reference()
  from spartan.array import extent
  from spartan.examples import lanczos as ref_lanczos
  from spartan.examples import spectral_clustering as ref
  p, truth = case.planted()
  n, d = p.shape
  out = dict(points=p, truth=truth)
  bands = [(b * n // BANDS, (b + 1) * n // BANDS) for b in range(BANDS)]
  point_tiles = [extent.create((lo, 0), (hi, d), p.shape) for lo, hi in bands]
  src = Points(p, point_tiles)
  for metric in case.METRICS:
    rows = []
    for ex in point_tiles:
      (_, a), = list(ref._row_similarity_mapper(src, ex, metric))
      rows.append(np.asarray(a, np.float64))
    a = np.vstack(rows)
    deg = a.sum(axis=1)
    a_tiles = [extent.create((lo, 0), (hi, n), (n, n)) for lo, hi in bands]
    a_src = Points(a, a_tiles)
    lap = np.vstack([np.asarray(list(ref._laplacian_mapper(a_src, ex, deg.copy()))[0][1], np.float64) for ex in a_tiles])
    assert a.shape == (n, n) and lap.shape == (n, n) and np.all(np.diag(lap) == 1)
    out['A_' + metric], out['D_' + metric], out['L_' + metric] = a, deg, lap
  lap = out['L_rbf']
  started = False
  try:
    mg.start_cluster(sp, WORKERS)
    started = True
    from spartan.config import FLAGS
    FLAGS.num_workers = WORKERS
    dd, ss = ref_lanczos.solve(sp.from_numpy(lap.copy()), sp.from_numpy(lap.copy()), RANK, True)
    print('spectral_w4.npz: lanczos.solve() evaluated at %d workers' % WORKERS)
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    print("spectral_w4.npz: the reference's lanczos.solve() did not evaluate:", type(e).__name__, str(e)[:400])
    dd, ss = ritz_pairs(lap.dot, n, RANK)
  dn, _ = ritz_pairs(lap.dot, n, RANK)           # the project's own host routine on numpy.dot
  np.testing.assert_allclose(np.real(dd), dn, rtol=1e-9, atol=0)
  out['lanczos_d'], out['lanczos_s'] = np.asarray(np.real(dd), np.float64), np.asarray(np.real(ss), np.float64)
  u = out['lanczos_s'][:, :K]
  labels = lloyd(u, u[np.argmax(u, axis=0)], NUM_ITER)
  out['labels'] = labels.astype(np.int64)
  assert case.partition(labels) == case.partition(truth), 'the composed run does not find the planted groups'
  if started:
    try:
      whole = ref.spectral_cluster(sp.from_numpy(p.copy()), K, NUM_ITER)
      whole = np.asarray(whole.glom()).reshape(-1).astype(np.int64)
      out['labels_w4'] = whole
      print('spectral_w4.npz: spectral_cluster() evaluated at %d workers' % WORKERS)
      assert case.partition(whole) == case.partition(truth), 'the whole run does not find the planted groups'
    except AssertionError:
      raise
    except Exception as e:   # noqa: BLE001
      print("spectral_w4.npz: the reference's spectral_cluster() did not evaluate:", type(e).__name__, str(e)[:400])
  path = os.path.join(HERE, 'spectral_w4.npz')
  np.savez_compressed(path, **out)
  print('spectral_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out))
  print('leading Ritz values:', out['lanczos_d'])


if __name__ == '__main__':
  main()
