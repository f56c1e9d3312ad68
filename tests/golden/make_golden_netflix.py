"""Records tests/golden/netflix_w4.npz: the reference's own Netflix SGD (spartan/examples/netflix.py, sgd, with its
compiled inner loop netflix_core.pyx) on the input of tests/netflix_cases.golden_input -- 52 users x 400 movies on a
4 x 4 grid, rank 20, about 1500 distinct ratings 1 .. 5, float32 -- for two epochs at 4 workers, with the helpers of
make_golden.py (the reference tree is copied to a scratch directory, transliterated to Python 3 there, its .pyx files
cythonized THERE and run in process; only the arrays are kept).

  python tests/golden/make_golden_netflix.py

  rows, cols, vals, U0, M0   the input
  U_1, M_1, U_2, M_2         the factors after epochs 1 and 2
  strata_blocks              [32, 2]: the blocks (bi, bj) in the order the reference's _compute_strata drew them,
  strata_sizes               blocks per stratum,
  strata_counts              strata per epoch (a new stratification is drawn every epoch; `random` is seeded)
  whole_run                  1 if the transliterated reference evaluated sgd(); 0 if the script had to call the
                             reference's _sgd_inner block by block in a recorded stratification (it prints what stopped
                             it)

Each tile reaches the reference as COO in row-major order: the script watches _sgd_inner and asserts it.  It also
asserts that the factors moved by at least 100 times the accuracy limit of tests/netflix_cases.py (8 e_ref), so that a
run that does nothing cannot pass."""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import netflix_cases as case  # noqa: E402


def build_core():
  """netflix_core.pyx of the scratch tree as an extension of this interpreter, beside the scratch copy."""
  from Cython.Build import cythonize
  from setuptools import Extension, setup
  os.chdir(mg.SCRATCH)
  ext = Extension('spartan.examples.netflix_core', ['spartan/examples/netflix_core.pyx'], include_dirs=[np.get_include()])
  setup(script_args=['build_ext', '--inplace', '-q'],
        ext_modules=cythonize([ext], language_level=2, quiet=True, compiler_directives={'always_allow_keywords': True}))


def _loader(inputs, ex, whole=None):
  import scipy.sparse
  block = whole[ex.ul[0]:ex.lr[0], ex.ul[1]:ex.lr[1]].tocoo()
  order = np.lexsort((block.col, block.row))
  yield ex, scipy.sparse.coo_matrix((block.data[order], (block.row[order], block.col[order])), shape=block.shape)


def main():
  import scipy.sparse
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  path = os.path.join(mg.SCRATCH, 'spartan', 'examples', 'netflix.py')
  text = open(path).read()
  if 'from netflix_core import' in text:            # (an implicit relative import)
    open(path, 'w').write(text.replace('from netflix_core import', 'from spartan.examples.netflix_core import'))
  build_core()
  mg.install_stubs()
  sp = mg.import_reference()
  from spartan.examples import netflix as ref

  rows, cols, vals, u0, m0 = case.golden_input()
  users, movies, grid, rank = case.USERS, case.MOVIES, case.GRID, case.RANK
  rcuts, ccuts = case.grid_cuts(users, grid), case.grid_cuts(movies, grid)
  out = {'rows': rows, 'cols': cols, 'vals': vals, 'U0': u0, 'M0': m0}

  # what the reference draws and what its inner loop is handed
  drawn, seen = [], []
  real_strata, real_inner = ref._compute_strata, ref._sgd_inner

  def watched_strata(V):
    strata = real_strata(V)
    drawn.append([[([c[0] for c in rcuts].index(ex.ul[0]), [c[0] for c in ccuts].index(ex.ul[1])) for ex in st]
                  for st in strata])
    return strata

  def watched_inner(r, c, v, u, m):
    assert r.dtype == c.dtype == np.int64 and v.dtype == u.dtype == m.dtype == np.float32
    key = r * (int(c.max()) + 1 if len(c) else 1) + c
    assert (np.diff(key) > 0).all(), 'a tile reached _sgd_inner out of row-major order, or with duplicates'
    seen.append(len(r))
    return real_inner(r, c, v, u, m)
  ref._compute_strata, ref._sgd_inner = watched_strata, watched_inner

  whole_mat = scipy.sparse.csr_matrix((vals, (rows, cols)), shape=(users, movies))
  random.seed(20150708)
  whole, results = 1, []
  try:
    mg.start_cluster(sp, case.WORKERS)
    from spartan.config import FLAGS
    FLAGS.num_workers = case.WORKERS
    V = sp.sparse_empty((users, movies), tile_hint=(rcuts[0][1], ccuts[0][1]), dtype=np.float32)
    V = sp.eager(sp.tocoo(sp.shuffle(V, _loader, target=V, kw={'whole': whole_mat})))
    M = sp.eager(sp.from_numpy(m0.copy(), tile_hint=(ccuts[0][1], rank)))
    U = sp.eager(sp.from_numpy(u0.copy(), tile_hint=(rcuts[0][1], rank)))
    for _ in range(case.EPOCHS):
      ref.sgd(V, M, U).evaluate()
      results.append((np.array(U.glom(), np.float32), np.array(M.glom(), np.float32)))
    assert len(drawn) == case.EPOCHS and sum(seen) == case.EPOCHS * len(vals), (len(drawn), sum(seen))
    print('netflix_w4.npz: sgd() evaluated at %d workers; %d calls of _sgd_inner' % (case.WORKERS, len(seen)))
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    print("netflix_w4.npz: the reference's sgd() did not evaluate:", type(e).__name__, str(e)[:400])
    whole, results = 0, []
    rnd = random.Random(20150708)
    drawn[:] = []
    u, m = u0.copy(), m0.copy()
    for _ in range(case.EPOCHS):
      blocks = [(i, j) for i in range(grid) for j in range(grid)]
      rnd.shuffle(blocks)
      strata = []
      while blocks:                                    # the reference's greedy pick
        st = []
        for b in list(blocks):
          if all(b[0] != o[0] and b[1] != o[1] for o in st):
            st.append(b)
        for b in st:
          blocks.remove(b)
        strata.append(st)
      drawn.append(strata)
      for st in strata:
        for bi, bj in st:
          (r0, r1), (c0, c1) = rcuts[bi], ccuts[bj]
          indptr, indices, bv = case.block(rows, cols, vals, rcuts[bi], ccuts[bj], np.float32)
          br = np.repeat(np.arange(r1 - r0), np.diff(indptr)).astype(np.int64)
          ub, mb = np.ascontiguousarray(u[r0:r1]), np.ascontiguousarray(m[c0:c1])
          real_inner(br, indices.astype(np.int64), bv, ub, mb)
          u[r0:r1], m[c0:c1] = ub, mb
      results.append((u.copy(), m.copy()))

  out['strata_blocks'] = np.asarray([b for ep in drawn for st in ep for b in st], np.int64).reshape(-1, 2)
  out['strata_sizes'] = np.asarray([len(st) for ep in drawn for st in ep], np.int64)
  out['strata_counts'] = np.asarray([len(ep) for ep in drawn], np.int64)
  for t, (u, m) in enumerate(results):
    out['U_%d' % (t + 1)], out['M_%d' % (t + 1)] = u, m
  out['whole_run'] = np.asarray(whole, np.int64)
  path = os.path.join(HERE, 'netflix_w4.npz')
  np.savez_compressed(path, **out)
  print('netflix_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out))

  # the recorded run against the float64 yardstick, and that it moved
  case._cache.clear()
  e_ref = case.e_ref()
  moved = max(float(np.abs(results[-1][0].astype(np.float64) - u0).max()), float(np.abs(results[-1][1].astype(np.float64) - m0).max()))
  print('netflix_w4.npz: e_ref = %.3g; the factors moved by up to %.3g = %.0f times the limit 8 e_ref'
        % (e_ref, moved, moved / (case.FACTOR * e_ref)))
  assert moved >= 100 * case.FACTOR * e_ref
  for dot in ('plain', 'stated'):
    got = case.epochs(lambda *a, dot=dot: case.restated(*a, dot=dot), rows, cols, vals, u0, m0, case.golden_strata())
    same = all(got[t][w].tobytes() == results[t][w].tobytes() for t in range(case.EPOCHS) for w in (0, 1))
    print('netflix_w4.npz: restated with the %s dot %s the recorded bytes' % (dot, 'equals' if same else 'does not equal'))


if __name__ == '__main__':
  main()
