"""Records tests/golden/lda_w4.npz: the reference's own LDA tile bodies (spartan/examples/lda.py, _lda_mapper and
_lda_doc_topic_mapper) and its whole learn_topics on the small input of tests/lda_cases.golden_input, with the helpers
of make_golden.py (the reference tree is copied to a scratch directory, transliterated to Python 3 there and run in
process; only the arrays are kept).

  python tests/golden/make_golden_lda.py

  x, n0             48 x 40 float64 counts (document 7 empty, term 11 in no document), 5 x 48 float64 starting counts
  train_whole_p{1,2}, doc_whole_p{1,2}
                    _lda_mapper (N + delta) and _lda_doc_topic_mapper (doc_topics) on the whole matrix with n0, for
                    max_iter_per_doc 1 and 2
  train_band{0..3}_p{1,2}, doc_band{0..3}_p{1,2}
                    the same on each of the four bands of 10 documents
  chain_counts{1,2}, chain_doc_topics, chain_counts_normalised
                    max_iter = 2, max_iter_per_doc = 1 composed by this script from the mappers on the four bands: every
                    band yields N + delta and the bands are added, N' = 4 N + sum of the deltas
  w4_doc_topics, w4_counts
                    the reference's whole learn_topics(x, 5, max_iter=2, max_iter_per_doc=1) at 4 workers with its
                    expr.rand replaced for the duration by a function that returns n0 -- if the transliterated reference
                    evaluates it; otherwise the script prints what stopped it

The script asserts that the whole run equals the composition (T . N + sum of the mapper outputs' deltas, T = 4 tiles
of documents): the behaviour the driver keeps is pinned to the reference's own output."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import lda_cases as case  # noqa: E402

WORKERS = 4
ALPHA, ETA = 0.1, 0.1


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  mg.install_stubs()
  sp = mg.import_reference()
  from spartan.array import extent
  from spartan.examples import lda as ref
  x, n0 = case.golden_input()
  v, d = x.shape
  k = n0.shape[0]
  out = dict(x=x, n0=n0)
  ex_n = extent.create((0, 0), n0.shape, n0.shape)
  bands = [(b * d // case.GOLDEN_BANDS, (b + 1) * d // case.GOLDEN_BANDS) for b in range(case.GOLDEN_BANDS)]

  def train(lo, hi, n, p):
    ex = extent.create((0, lo), (v, hi), x.shape)
    (_, counts), = list(ref._lda_mapper(ex, x[:, lo:hi].copy(), ex_n, n.copy(), k, ALPHA, ETA, p))
    return np.asarray(counts, np.float64)

  def infer(lo, hi, n, p):
    ex = extent.create((0, lo), (v, hi), x.shape)
    (_, doc_topics), = list(ref._lda_doc_topic_mapper(ex, x[:, lo:hi].copy(), ex_n, n.copy(), k, ALPHA, ETA, p))
    return np.asarray(doc_topics, np.float64)

  with np.errstate(all='ignore'):
    for p in (1, 2):
      out['train_whole_p%d' % p], out['doc_whole_p%d' % p] = train(0, d, n0, p), infer(0, d, n0, p)
      for b, (lo, hi) in enumerate(bands):
        out['train_band%d_p%d' % (b, p)], out['doc_band%d_p%d' % (b, p)] = train(lo, hi, n0, p), infer(lo, hi, n0, p)
    n1 = sum(out['train_band%d_p1' % b] for b in range(len(bands)))
    n2 = sum(train(lo, hi, n1, 1) for lo, hi in bands)
    out['chain_counts1'], out['chain_counts2'] = n1, n2
    out['chain_doc_topics'] = np.vstack([infer(lo, hi, n2, 1) for lo, hi in bands])
    out['chain_counts_normalised'] = n2 / np.abs(n2).sum(axis=1)[:, None]
  assert np.isnan(out['doc_whole_p1'][7]).all() and not np.isnan(np.delete(out['doc_whole_p1'], 7, axis=0)).any()
  assert np.array_equal(out['train_whole_p1'][:, 11], n0[:, 11])
  try:
    mg.start_cluster(sp, WORKERS)
    from spartan.config import FLAGS
    FLAGS.num_workers = WORKERS
    keep = ref.expr.rand
    ref.expr.rand = lambda *shape, **kw: sp.from_numpy(n0.copy())
    try:
      doc_topics, counts = ref.learn_topics(sp.from_numpy(x.copy()), k, alpha=ALPHA, eta=ETA, max_iter=2, max_iter_per_doc=1)
      doc_topics, counts = np.asarray(doc_topics.glom(), np.float64), np.asarray(counts.glom(), np.float64)
    finally:
      ref.expr.rand = keep
    out['w4_doc_topics'], out['w4_counts'] = doc_topics, counts
    print('lda_w4.npz: learn_topics() evaluated at %d workers' % WORKERS)
    np.testing.assert_allclose(counts, out['chain_counts_normalised'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(doc_topics, out['chain_doc_topics'], rtol=1e-12, atol=0)
    print('lda_w4.npz: the whole run equals 4 . N + the sum of the four bands\' deltas, iteration by iteration')
  except AssertionError:
    raise
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    print("lda_w4.npz: the reference's learn_topics() did not evaluate:", type(e).__name__, str(e)[:400])
  path = os.path.join(HERE, 'lda_w4.npz')
  np.savez_compressed(path, **out)
  print('lda_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out))


if __name__ == '__main__':
  main()
