"""Records tests/golden/swaption_w4.npz: the reference's own swaption pricer (spartan/examples/swaption.py, simulate) on
the 16 products of its benchmark (tests/benchmark_swaption.py) with NUM_PATHS = 10 -- the one value its two
reshape((20, )) admit -- at 4 workers, with the helpers of make_golden.py (the reference tree is copied to a scratch
directory, transliterated to Python 3 there and run in process; only the arrays are kept).

  python tests/golden/make_golden_swaption.py

  products        [16, 3]: (ts, te, lamb) in simulate's iteration order
  eps_00 .. 15    [S, 10] each: the product's draws.  The script watches the module's `randn`: every array it makes is
                  evaluated where it is made, copied, and handed on as the evaluated array (so that the program prices
                  the very draws that are kept)
  results         [16, 2]: the [mean, std] simulate returns, in basis points
  whole_run       1 if the transliterated reference evaluated simulate; 0 if the script had to compose the arrays with
                  the literal NumPy float64 transcription of its program (tests/swaption_cases.oracle) on draws of
                  NumPy's generator (it prints what stopped it)

The run recorded here has whole_run = 0.  Two things stop the reference at this revision: its arange call (below: as
written both structures have length 0 and the first assign asserts), and, with that call given its stated meaning, a
map of the first time step at 4 workers that fetches rows 2:3 of a 2-row operand ("Requested region is out of
bounds", map.py:276 -- the join of the sliced plane with the broadcast row of draws).

The script asserts that the recorded results agree with the transcription on the recorded draws to 1e-9 relative."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import swaption_cases as case  # noqa: E402

SEED = 20151107


def _composed(eps, te, lamb):
  v = case.oracle(eps, case.steps_of(1, te)[1], lamb)
  return [v.mean() * 10000, v.std() / np.sqrt(len(v)) * 10000]


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  mg.install_stubs()
  sp = mg.import_reference()
  products = case.products()
  n = case.NUM_PATHS
  draws = []
  whole = 1
  try:
    mg.start_cluster(sp, case.WORKERS)
    from spartan.config import FLAGS
    FLAGS.num_workers = case.WORKERS
    import spartan
    from spartan.examples import swaption as ref
    assert (ref.DELTA, ref.F_0, ref.THETA) == (case.DELTA, case.F_0, case.THETA)
    real_randn = ref.randn

    def watched_randn(*shape, **kw):
      made = real_randn(*shape, **kw).evaluate()
      draws.append(np.array(made.glom(), np.float64))
      return spartan.expr.lazify(made)
    ref.randn = watched_randn
    # swaption.py calls arange(None, 0, ts + DELTA, DELTA) -- (shape, start, stop, step), an earlier signature.  The
    # reference's arange is (start, stop, step, dtype): as written the call means start = 0, stop = 0, step = ts + DELTA,
    # dtype = DELTA, both structures have length 0 and simulate stops at its first assign.  The call is given the
    # meaning its argument order states.
    real_arange = ref.arange
    ref.arange = lambda shape, start, stop, step: real_arange(start, stop, step)
    np.random.seed(SEED)
    got = ref.simulate(case.TS_ALL, case.TE_ALL, case.LAMB_ALL, n)
    results = np.asarray([[float(np.asarray(me.glom())), float(np.asarray(st.glom()))] for me, st in got], np.float64)
    assert len(draws) == len(products) == len(results)
    print('swaption_w4.npz: simulate() evaluated at %d workers' % case.WORKERS)
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    import traceback
    where = ['%s:%d %s' % (os.path.relpath(f.filename, mg.SCRATCH), f.lineno, f.line) for f in traceback.extract_tb(e.__traceback__)[-4:]]
    print("swaption_w4.npz: the reference's simulate() did not evaluate:", type(e).__name__, str(e)[:400], where)
    whole = 0
    rng = np.random.RandomState(SEED)
    draws = [rng.randn(case.steps_of(ts, te)[0], n) for ts, te, _ in products]
    results = np.asarray([_composed(eps, te, lamb) for eps, (_, te, lamb) in zip(draws, products)], np.float64)

  for i, (eps, (ts, te, lamb)) in enumerate(zip(draws, products)):
    assert eps.shape == (case.steps_of(ts, te)[0], n) and np.isfinite(eps).all(), (i, eps.shape)
    np.testing.assert_allclose(results[i], _composed(eps, te, lamb), rtol=1e-9, atol=0, err_msg=str((i, ts, te, lamb)))
  assert (results > 0).all()
  out = {'products': np.asarray(products, np.float64), 'results': results, 'whole_run': np.asarray(whole, np.int64)}
  out.update(('eps_%02d' % i, eps) for i, eps in enumerate(draws))
  print('swaption_w4.npz: means %s bp' % np.array2string(results[:, 0], precision=1))
  path = os.path.join(HERE, 'swaption_w4.npz')
  np.savez_compressed(path, **out)
  print('swaption_w4.npz:', os.path.getsize(path), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
  main()
