"""Records tests/golden/nb_w4.npz: the reference's own naive Bayes (spartan/examples/naive_bayes.py,
_sum_instance_by_label_mapper, fit and predict) on the small input of tests/nb_cases.golden_input, with the helpers of
make_golden.py (the reference tree is copied to a scratch directory, transliterated to Python 3 there and run in
process; only the arrays are kept).

  python tests/golden/make_golden_nb.py

  data, labels, queries   120 x 24 float64 counts, int64 labels in 0 .. 3, 10 one-row queries
  df, idf, rms            the reference's formulas (naive_bayes.py:37-53) in NumPy float64
  W                       _sum_instance_by_label_mapper on the four bands of 30 rows of the reference-normalised data
                          (data / rms * idf), the four outputs added in band order
  wl                      W.sum(axis=1)
  scores, scores_per_label
                          both outputs of the reference's whole fit(data, labels, 4) at 4 workers -- if the
                          transliterated reference evaluates it; otherwise the script prints what stopped it and
                          records the composition of the recorded pieces, log((W + 1) / (wl + 24)) and wl
  whole_fit               1 if the two were recorded from the whole fit, 0 if composed
  predicted               predict(model, query) for the 10 queries (the reference's if the whole fit evaluated,
                          else argmax(scores . query))

The script asserts the shape of the input (no row of zeros, every label in every band) and that for every query the two
best scores differ by at least 1e-3 relative -- far above the float32 bound -- so a float32 run must find the same
labels."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import nb_cases as case  # noqa: E402

WORKERS = 4
BANDS = 4
ALPHA = 1.0


class Rows(object):
  """What the reference's mapper asks of a distributed array: shape and fetch."""

  def __init__(self, data):
    self.data, self.shape = data, data.shape

  def fetch(self, ex):
    return self.data[ex.to_slice()]


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  mg.install_stubs()
  sp = mg.import_reference()
  from spartan.array import extent
  from spartan.examples import naive_bayes as ref
  data, labels, label_size, queries = case.golden_input()
  n, d = data.shape
  bands = [(b * n // BANDS, (b + 1) * n // BANDS) for b in range(BANDS)]
  assert data.dtype == np.float64 and np.all(data >= 0) and np.all(data == np.round(data))
  assert np.all((data != 0).any(axis=1)), 'a row of zeros'
  for lo, hi in bands:
    assert set(labels[lo:hi].tolist()) == set(range(label_size)), 'a band without one of the labels'

  df = (data > 0).sum(axis=0)
  idf = np.log(n * 1.0 / (df + 1)) + 1
  rms = np.sqrt(np.square(data).sum(axis=1) * 1.0 / d)
  normalised = data / rms.reshape((n, 1)) * idf.reshape((1, d))
  src, lab = Rows(normalised), Rows(labels.reshape(n, 1))
  w = np.zeros((label_size, d))
  for lo, hi in bands:
    (_, part), = list(ref._sum_instance_by_label_mapper(src, extent.create((lo, 0), (hi, d), (n, d)), lab, label_size))
    w = w + np.asarray(part, np.float64)
  wl = w.sum(axis=1)
  out = dict(data=data, labels=labels, queries=queries, df=df.astype(np.int64), idf=idf, rms=rms, W=w, wl=wl)
  model = None
  try:
    mg.start_cluster(sp, WORKERS)
    from spartan.config import FLAGS
    FLAGS.num_workers = WORKERS
    model = ref.fit(sp.from_numpy(data.copy(), tile_hint=(n // BANDS, d)),
                    sp.from_numpy(labels.reshape(n, 1).copy(), tile_hint=(n // BANDS, 1)), label_size, ALPHA)
    scores = np.asarray(model['scores_per_label_and_feature'].glom(), np.float64)
    per_label = np.asarray(model['scores_per_label'].glom(), np.float64).reshape(-1)
    predicted = [int(ref.predict(model, sp.from_numpy(q.reshape(1, d).copy()))) for q in queries]
    print('nb_w4.npz: fit() and predict() evaluated at %d workers' % WORKERS)
    whole = 1
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    print("nb_w4.npz: the reference's fit() did not evaluate:", type(e).__name__, str(e)[:400])
    scores = np.log((w + ALPHA) / (wl.reshape((label_size, 1)) + ALPHA * d))
    per_label = wl
    predicted = [int(np.argmax(scores.dot(q.reshape(d, 1)))) for q in queries]
    whole = 0
  composed = np.log((w + ALPHA) / (wl.reshape((label_size, 1)) + ALPHA * d))
  np.testing.assert_allclose(scores, composed, rtol=1e-12, atol=0)
  np.testing.assert_allclose(per_label, wl, rtol=1e-12, atol=0)
  gaps = []
  for q, p in zip(queries, predicted):
    v = np.sort(scores.dot(q))
    gaps.append(float((v[-1] - v[-2]) / abs(v[-1])))
    assert p == int(np.argmax(scores.dot(q)))
  print('nb_w4.npz: the two best scores of a query differ by at least %.3g relative; predicted %s' % (min(gaps), predicted))
  assert min(gaps) >= 1e-3
  out.update(scores=scores, scores_per_label=per_label, predicted=np.asarray(predicted, np.int64),
             whole_fit=np.asarray(whole, np.int64),
             predicted_rows=np.argmax(data.dot(scores.T), axis=1).astype(np.int64))
  rows = np.sort(data.dot(scores.T), axis=1)
  print('nb_w4.npz: over the 120 rows the two best scores differ by at least %.3g relative'
        % float(((rows[:, -1] - rows[:, -2]) / np.abs(rows[:, -1])).min()))
  assert float(((rows[:, -1] - rows[:, -2]) / np.abs(rows[:, -1])).min()) >= 1e-3
  path = os.path.join(HERE, 'nb_w4.npz')
  np.savez_compressed(path, **out)
  print('nb_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out))


if __name__ == '__main__':
  main()
