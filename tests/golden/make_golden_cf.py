"""Records tests/golden/item_recommender_w4.npz: the reference's own ItemBasedRecommender
(spartan/examples/cf/item_recommender.py, precompute) on the table of tests/cf_cases.golden_input -- 40 users x 24 items,
float64, about 30 % filled, negative ratings included, item 7 rated by nobody -- as a csr sparse array (what its own
test feeds it) at 4 workers with k = 5, with the helpers of make_golden.py (the reference tree is copied to a scratch
directory, transliterated to Python 3 there and run in process; only the arrays are kept).

  python tests/golden/make_golden_cf.py

  table                   [40, 24] the table's dense form
  item_norm               [24]     the reference's _get_norm_of_each_item
  similarity_table        [24, 24] the reference's N x N table, glommed BEFORE its second shuffle selects from it
  top_k_similar_table     [24, 5]  } the reference's results, every row re-sorted HERE by (value descending, index
  top_k_similar_indices   [24, 5]  } ascending): the reference leaves a row in the order its quick-select stops in
  as_written_indices      [24, 5]  top_k_similar_indices of the reference's UNMODIFIED precompute(); -1 throughout if
                                   that run does not evaluate (the script prints what stopped it)
  whole_run               1 if the transliterated reference evaluated precompute() with its own Cython helper
                          (cf/helper.pyx argpartsort, cythonized in the scratch copy) under the two repairs below; 0 if
                          the script had to replace that helper by a NumPy restatement (argpartition), or compose the
                          arrays in NumPy float64 altogether -- the script prints what stopped it

The four result arrays come from the reference's own precompute() with two repairs made in this script, because as
written its second shuffle does not compute what its docstring states (as_written_indices records what it does: in the
recording run no row held the indices of its k most similar items):
  1. argpartsort selects on a COPY of the tile.  The helper says "Sort original array, no copy" and permutes the
     similarity tile in place while it permutes its index array; the mapper then reads the values
     `local_similarity_table[i, sorted_indices[i]]` from the permuted tile at the original positions, so values and
     indices no longer belong together (and similarity_table itself is left permuted).  bottleneck's original copies.
  2. the second shuffle gets the table in whole rows (retiled to (N / workers, N)).  The first shuffle's updates leave
     similarity_table in (band x step) tiles -- 6 x 6 here -- and _select_most_k_similar_mapper treats every tile as
     if it held whole rows: it selects among the tile's 6 columns, reports tile-local column numbers and every column
     block of a row band overwrites the same (band, k) target.
Both repairs implement what its docstrings state ("Find the top k similar items for each item").

The script asserts that in every row but the all-zero item's the k-th and (k + 1)-th largest similarities differ by
more than twice the derived float64 driver bound of tests/cf_cases.py (the seed of golden_input was chosen so that
this holds): the reference's index SETS are then unambiguous and no row has to be left out of a comparison.  The
all-zero item's own row ties at 0 throughout, by construction; tests compare its values and assert our stated tie
order for it."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import cf_cases as case  # noqa: E402

WORKERS = 4


def prepare_cf():
  """lib2to3 over the reference's cf package in the scratch copy, and its helper.pyx cythonized there."""
  os.chdir(mg.SCRATCH)
  d = 'spartan/examples/cf'
  files = [os.path.join(d, f) for f in os.listdir(d) if f.endswith('.py')]
  subprocess.check_call([sys.executable, '-m', 'lib2to3', '-w', '-n', '-x', 'map', '-x', 'filter', '-x', 'reduce', '-x', 'zip',
                         '-x', 'import'] + files, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
  for f in files:
    t = open(f).read()
    t2 = t.replace('dtype=np.int)', 'dtype=np.int64)')           # (np.int: an alias NumPy has removed)
    t2 = t2.replace('from item_recommender import', 'from .item_recommender import')    # (a Python-2 implicit relative import)
    if t2 != t:
      open(f, 'w').write(t2)
  # the helper calls np.array with only the C-level numpy cimported: Cython 0.x fell back to the Python module
  pyx = os.path.join(d, 'helper.pyx')
  t = open(pyx).read()
  if '\nimport numpy as np\n' not in t:
    mg.sub(pyx, [('cimport numpy as np\n', 'cimport numpy as np\nimport numpy as np\n')])


def build_helper():
  from Cython.Build import cythonize
  from setuptools import Extension, setup
  os.chdir(mg.SCRATCH)
  exts = [Extension('spartan.examples.cf.helper', ['spartan/examples/cf/helper.pyx'], include_dirs=[np.get_include()])]
  setup(script_args=['build_ext', '--inplace', '-q'],
        ext_modules=cythonize(exts, language_level=2, quiet=True, compiler_directives={'always_allow_keywords': True}))


def _argpartsort_numpy(arr, n, axis=1):
  """What the helper is documented to return: indices that put the n LARGEST of every row first, in no order."""
  assert axis == 1
  arr = np.asarray(arr)
  return np.argpartition(-arr, min(n, arr.shape[1]) - 1, axis=1)


def _composed(table, k):
  """The reference's arithmetic in NumPy float64: norms, table, quick-selected top k."""
  norm = np.sqrt((table * table).sum(axis=0))
  with np.errstate(all='ignore'):
    sim = np.nan_to_num(table.T.dot(table) / norm[:, None].dot(norm[None, :]))
  idx = _argpartsort_numpy(sim, k)[:, :k]
  return norm, sim, np.take_along_axis(sim, idx, axis=1), idx


def main():
  import scipy.sparse
  table = np.array(case.golden_input())
  users, n = table.shape
  k = case.GOLDEN_K
  assert (users, n, k) == (40, 24, 5) and not table[:, case.GOLDEN_ZERO_ITEM].any()
  fill = np.count_nonzero(table) / float(table.size)
  assert 0.2 < fill < 0.4 and (table < 0).any(), fill
  assert case.golden_gaps_are_clear(table, k), 'choose another GOLDEN_SEED: a row ties at the cut'

  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  prepare_cf()
  helper_built = True
  try:
    build_helper()
  except BaseException as e:   # noqa: BLE001  (setup() may exit)
    print('item_recommender_w4.npz: cf/helper.pyx did not build:', type(e).__name__, str(e)[:300])
    helper_built = False
  os.chdir(mg.SCRATCH)
  mg.install_stubs()
  sp = mg.import_reference()

  whole = 1
  as_written_idx = np.full((n, k), -1, np.int64)
  try:
    mg.start_cluster(sp, WORKERS)
    from spartan.config import FLAGS
    FLAGS.num_workers = WORKERS
    if not helper_built:
      import types
      stand_in = types.ModuleType('spartan.examples.cf.helper')
      stand_in.argpartsort = _argpartsort_numpy
      sys.modules['spartan.examples.cf.helper'] = stand_in
      whole = 0
    from spartan.examples.cf import item_recommender as ref
    in_place = ref.argpartsort
    real_expr = ref.expr
    seen = {}

    class Repaired(object):
      """The reference's `expr` module with the second shuffle of precompute() given whole rows (repair 2)."""

      def __getattr__(self, name):
        return getattr(real_expr, name)

      def shuffle(self, array, fn, *args, **kw):
        if fn is ref._select_most_k_similar_mapper:
          seen['similarity_table'] = np.array(array.glom(), np.float64)          # (before anything selects from it)
          array = real_expr.retile(array, tile_hint=(n // WORKERS, n))
        return real_expr.shuffle(array, fn, *args, **kw)

    def run():
      rating = sp.from_numpy(scipy.sparse.csr_matrix(table), tile_hint=(users, n // WORKERS))
      model = ref.ItemBasedRecommender(rating, k)
      norm = np.asarray(model._get_norm_of_each_item(model.rating_table).glom(), np.float64).reshape(n)
      model.precompute()
      return model, norm

    ref.expr = Repaired()
    ref.argpartsort = lambda arr, n_, axis=1: in_place(np.array(arr), n_, axis)     # (repair 1: select on a copy)
    try:
      model, norm = run()
    except Exception as e:   # noqa: BLE001
      if not whole:
        raise
      print('item_recommender_w4.npz: precompute() with the Cython helper did not evaluate (%s: %s); the helper is '
            'replaced by a NumPy restatement' % (type(e).__name__, str(e)[:300]))
      ref.argpartsort = _argpartsort_numpy
      whole = 0
      model, norm = run()
    sim = seen['similarity_table']
    top = np.asarray(model.top_k_similar_table, np.float64)
    idx = np.asarray(model.top_k_similar_indices, np.int64)
    print('item_recommender_w4.npz: precompute() evaluated at %d workers (whole_run = %d)' % (WORKERS, whole))
    # ... and the reference as written (last: whatever it does to the cluster, nothing runs after it)
    ref.expr, ref.argpartsort = real_expr, in_place
    try:
      model, _ = run()
      as_written_idx = np.asarray(model.top_k_similar_indices, np.int64).reshape(n, k)
    except Exception as e:   # noqa: BLE001
      print('item_recommender_w4.npz: precompute() AS WRITTEN did not evaluate (as_written_indices is -1):',
            type(e).__name__, str(e)[:200])
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    print("item_recommender_w4.npz: the reference's precompute() did not evaluate:", type(e).__name__, str(e)[:400])
    whole = 0
    norm, sim, top, idx = _composed(table, k)

  # what was recorded is the reference's arithmetic on this table
  c_norm, c_sim, _, _ = _composed(table, k)
  np.testing.assert_allclose(norm, c_norm, rtol=1e-12, atol=0)
  np.testing.assert_allclose(sim, c_sim, rtol=0, atol=1e-12)
  assert top.shape == (n, k) and idx.shape == (n, k)
  assert np.array_equal(np.take_along_axis(sim, idx, axis=1), top)          # the values are the table's at the indices
  for j in range(n):                                                          # ... and they are a row's k largest
    assert len(set(idx[j].tolist())) == k and top[j].min() >= np.sort(sim[j])[::-1][k - 1], j
  top, idx = case.rows_by_order(top, idx)
  out = dict(table=table, item_norm=norm, similarity_table=sim, top_k_similar_table=top, top_k_similar_indices=idx,
             whole_run=np.asarray(whole, np.int64), as_written_indices=as_written_idx)
  path = os.path.join(HERE, 'item_recommender_w4.npz')
  np.savez_compressed(path, **out)
  truth = [set(r.tolist()) for r in idx]
  print('item_recommender_w4.npz: as written, %d of %d rows hold the indices of their k most similar items; its rows 0, 1: %s'
        % (sum(set(r.tolist()) == t for r, t in zip(as_written_idx, truth)), n, as_written_idx[:2].tolist()))
  print('item_recommender_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out), '; fill %.2f' % fill)


if __name__ == '__main__':
  main()
