"""Records tests/golden/isomap_w4.npz: the reference's own shortest-path step (spartan/examples/sklearn/util/
graph_shortest_path.pyx, Dijkstra on a Fibonacci heap, undirected) on the neighbour graph of tests/test_isomap_example.py
-- the 200-point S-curve in float64, 8 neighbours -- with the helpers of make_golden.py (the reference tree is copied
to a scratch directory, transliterated to Python 3 there, its Cython compiled there and run in process; only the arrays
are kept).

  python tests/golden/make_golden_isomap.py

  x               the input
  dist_matrix     graph_shortest_path(kng, row_beg, row_end, directed=False) over the four row bands four workers take
                  (isomap.py:_shortest_path_mapper), summed as the reference's reducer sums them; kng is scikit-learn's
                  kneighbors_graph(mode='distance'), as in the reference
  fit_embedding   embedding_ of the reference's whole Isomap(8, 2, 'dense').fit at 4 workers (scikit-learn's neighbours
                  and KernelPCA around the step above), if the transliterated reference evaluates it -- it does once its
                  package's implicit relative import and the integer `/` of its tile_hint are patched in the scratch
                  copy; otherwise the script says what stopped it.  fit_dist_matrix is kept only if that run's
                  dist_matrix_ differs from dist_matrix (it does not).
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import test_isomap_example as case  # noqa: E402

WORKERS = 4


def prepare_manifold():
  """lib2to3 over the manifold driver and its util package (prepare_examples stops at sklearn/cluster), and the Cython
  build of graph_shortest_path.pyx in the scratch tree."""
  os.chdir(mg.SCRATCH)
  files = []
  for d in ('spartan/examples/sklearn/manifold', 'spartan/examples/sklearn/util'):
    files += [os.path.join(d, f) for f in os.listdir(d) if f.endswith('.py')]
  subprocess.check_call([sys.executable, '-m', 'lib2to3', '-w', '-n', '-x', 'map', '-x', 'filter', '-x', 'reduce',
                         '-x', 'zip', '-x', 'import'] + files, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
  # (the package's Python-2 implicit relative import; `/` on integers in the driver's tile_hint)
  init = 'spartan/examples/sklearn/manifold/__init__.py'
  if 'from isomap import' in open(init).read():
    mg.sub(init, [('from isomap import Isomap', 'from .isomap import Isomap')])
  drv = 'spartan/examples/sklearn/manifold/isomap.py'
  if 'n_points / n_workers' in open(drv).read():
    mg.sub(drv, [('n_points / n_workers', 'n_points // n_workers')])
  from Cython.Build import cythonize
  from setuptools import Extension, setup
  ext = Extension('spartan.examples.sklearn.util.graph_shortest_path',
                  ['spartan/examples/sklearn/util/graph_shortest_path.pyx'], include_dirs=[np.get_include()])
  setup(script_args=['build_ext', '--inplace', '-q'], ext_modules=cythonize([ext], language_level=2, quiet=True))


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  prepare_manifold()
  mg.install_stubs()
  sp = mg.import_reference()
  from sklearn.neighbors import NearestNeighbors, kneighbors_graph
  from spartan.examples.sklearn.util.graph_shortest_path import graph_shortest_path
  x = np.array(case.s_curve(np.float64))
  n = x.shape[0]
  kng = kneighbors_graph(NearestNeighbors(n_neighbors=case.K).fit(x), case.K, mode='distance')
  dist = np.zeros((n, n))
  for w in range(WORKERS):                     # the row bands of the reference's task array at 4 workers
    dist += graph_shortest_path(kng, w * n // WORKERS, (w + 1) * n // WORKERS, directed=False)
  assert np.all(dist[~np.eye(n, dtype=bool)] > 0), 'the neighbour graph is not connected'
  assert np.array_equal(dist, dist.T) or np.allclose(dist, dist.T, rtol=1e-14, atol=0)
  out = dict(x=x, dist_matrix=dist)
  try:
    from spartan.config import FLAGS
    from spartan.examples.sklearn.manifold.isomap import Isomap
    mg.start_cluster(sp, WORKERS)
    FLAGS.num_workers = WORKERS
    iso = Isomap(n_neighbors=case.K, n_components=2, eigen_solver='dense').fit(x)
    fd, fe = np.asarray(iso.dist_matrix_, np.float64), np.asarray(iso.embedding_, np.float64)
    print('isomap_w4.npz: Isomap.fit evaluated: dist_matrix_', fd.shape, 'embedding_', fe.shape,
          'same dist_matrix_ as the bands:', bool(np.array_equal(fd, dist)))
    out.update(fit_embedding=fe)
    if not np.array_equal(fd, dist):          # (otherwise the same 320 KB twice)
      out.update(fit_dist_matrix=fd)
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    print("isomap_w4.npz: the reference's Isomap.fit did not evaluate:", type(e).__name__, str(e)[:400])
  path = os.path.join(HERE, 'isomap_w4.npz')
  np.savez_compressed(path, **out)
  print('isomap_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out))


if __name__ == '__main__':
  main()
