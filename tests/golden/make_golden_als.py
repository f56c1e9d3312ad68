"""Records tests/golden/als_w4.npz: the reference's own ALS tile body (spartan/examples/als.py, _solve_U_or_M_mapper:
a loop over rows around scipy.linalg.lstsq) on the small rating matrix of tests/test_als_example.py, with the helpers
of make_golden.py (the reference tree is copied to a scratch directory, transliterated to Python 3 there and run in
process; only the arrays are kept).

  python tests/golden/make_golden_als.py

  A                 24 x 40 integer ratings in 0 .. 4, user row 3 all zero, no item column all zero
  M0                40 x 6 starting item factors: rand, column 0 the items' average rating (what the reference's als
                    assigns there, so that its run from `rand` = M0 and ours from M = M0 start alike)
  {explicit,implicit}_{U1,M1,U2,M2}
                    the mapper's outputs chained by this script: U1 = solve(A, M0), M1 = solve(A^T, U1), U2 = solve(A, M1),
                    M2 = solve(A^T, U2); la = 0.065, alpha = 40
  {explicit,implicit}_als_{U,M}
                    the reference's whole als(A, num_features=6, num_iter=2) at 4 workers with the scratch module's
                    expr.rand replaced at run time by one that returns M0, if the transliterated reference evaluates
                    it; otherwise the script prints what stopped it
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import test_als_example as case  # noqa: E402

WORKERS = 4


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  drv = 'spartan/examples/als.py'
  if 'np.float)' in open(drv).read():                      # (the removed alias of float64)
    mg.sub(drv, [('dtype=np.float)', 'dtype=np.float64)')])
  mg.install_stubs()
  sp = mg.import_reference()
  from spartan.array import extent
  from spartan.examples import als as ref
  a, m0 = case.ratings(), case.start_factors()
  out = dict(A=a, M0=m0)

  def solve(r, y, implicit):
    r = np.ascontiguousarray(r, dtype=np.float64)
    ex_a = extent.create((0, 0), r.shape, r.shape)
    ex_b = extent.create((0, 0), y.shape, y.shape)
    (_, result), = list(ref._solve_U_or_M_mapper(ex_a, r, ex_b, y, case.LA, case.ALPHA, implicit,
                                                 shape=(r.shape[0], y.shape[1])))
    return np.asarray(result, np.float64)

  for name, implicit in (('explicit', False), ('implicit', True)):
    u1 = solve(a, m0, implicit)
    m1 = solve(a.T, u1, implicit)
    u2 = solve(a, m1, implicit)
    m2 = solve(a.T, u2, implicit)
    out.update({name + '_U1': u1, name + '_M1': m1, name + '_U2': u2, name + '_M2': m2})
    try:
      mg.start_cluster(sp, WORKERS)
      from spartan.config import FLAGS
      FLAGS.num_workers = WORKERS
      real_rand = ref.expr.rand
      ref.expr.rand = lambda *shape, **kw: sp.from_numpy(m0.copy())
      try:
        u, m = ref.als(sp.from_numpy(a.astype(np.float64)), la=case.LA, alpha=case.ALPHA, implicit_feedback=implicit,
                       num_features=m0.shape[1], num_iter=2)
        u, m = np.asarray(u.glom(), np.float64), np.asarray(m.glom(), np.float64)
      finally:
        ref.expr.rand = real_rand
      print('als_w4.npz: %s als() evaluated at %d workers; max |U - U2| = %.3g, max |M - M2| = %.3g'
            % (name, WORKERS, np.abs(u - u2).max(), np.abs(m - m2).max()))
      out.update({name + '_als_U': u, name + '_als_M': m})
    except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
      print("als_w4.npz: the reference's als() (%s) did not evaluate:" % name, type(e).__name__, str(e)[:400])
  path = os.path.join(HERE, 'als_w4.npz')
  np.savez_compressed(path, **out)
  print('als_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out))


if __name__ == '__main__':
  main()
