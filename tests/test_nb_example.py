"""examples/naive_bayes: the naive Bayes driver.  CPU leg: the host framework on the injected NumPy backend, where the
tile body is the NumPy restatement beside the driver (examples/_nb.py).  GPU leg: the same checks on the HIP backend
(sp_nb_step), called from tests/test_nb_gpu.py.

Input and yardstick: tests/golden/nb_w4.npz, recorded by tests/golden/make_golden_nb.py from the reference's own fit at
4 workers on 120 documents x 24 terms with 4 labels (tests/nb_cases.golden_input); the script asserts that the two best
scores of every query and of every training row differ by at least 1e-3 relative -- far above the float32 bound -- so
a float32 run must find the same labels.

df is compared exactly.  Scores and weights: within bound(T, 'after') + bound(float64, 'inside') per entry
(tests/nb_cases.fit_bound: our error against the exact value plus the reference's own, which multiplies by idf inside
the sum); measured against bound is printed.  The shuffle must ask the kernel once per row band and never for anything
of size n x d: the backend's nb_step is watched."""
import functools
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples import naive_bayes as nb
from tests import nb_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))
ALPHA = 1.0


@functools.lru_cache(maxsize=None)
def golden():
  g = dict(np.load(os.path.join(HERE, 'golden', 'nb_w4.npz')))
  data, labels, label_size, queries = nc.golden_input()
  assert g['data'].tobytes() == data.tobytes() and g['labels'].tobytes() == labels.tobytes()
  assert g['queries'].tobytes() == queries.tobytes() and label_size == 4
  return g


@functools.lru_cache(maxsize=None)
def bounds(dtype):
  """(the fit's oracle, per output what |ours - golden| may be in `dtype`)."""
  data, labels, label_size, _ = nc.golden_input()
  want = nc.fit_oracle(data, labels, label_size, ALPHA)
  ours = nc.fit_bound(want, data.shape, ALPHA, dtype, 'after')
  theirs = nc.fit_bound(want, data.shape, ALPHA, np.float64, 'inside')
  return want, {k: ours[k] + theirs[k] for k in ours}


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _watch(ctx, asked):
  """Record what the driver asks of backend.nb_step (where the backend has one); returns the undo."""
  step = getattr(ctx.backend, 'nb_step', None)
  if step is None:
    return lambda: None

  def watched(x, labels, label_size, splits=0):
    asked.append((tuple(x.shape), tuple(labels.shape), label_size))
    return step(x, labels, label_size, splits=splits)
  ctx.backend.nb_step = watched

  def undo():
    del ctx.backend.nb_step
  return undo


def check_driver(backend, workers, dtype, labels_2d=True):
  g = golden()
  dt = np.dtype(dtype)
  data, labels, label_size, queries = nc.golden_input()
  n, d = data.shape
  ctx = _start(backend, workers)
  try:
    x = data.astype(dt)
    y = labels.reshape(n, 1) if labels_2d else labels
    hint_y = (n // workers, 1) if labels_2d else (n // workers,)
    X = sp.from_numpy(x, tile_hint=(n // workers, d)) if workers > 1 else sp.from_numpy(x)
    Y = sp.from_numpy(y, tile_hint=hint_y) if workers > 1 else sp.from_numpy(y)
    asked = []
    undo = _watch(ctx, asked)
    allocated = []
    empty = getattr(ctx.backend, 'empty', None)
    if empty is not None:                      # watch what is allocated while the model is fitted
      def watched_empty(shape, dtype):
        allocated.append(tuple(shape))
        return empty(shape, dtype)
      ctx.backend.empty = watched_empty
    try:
      model = nb.fit(X, Y, label_size, ALPHA)
    finally:
      if empty is not None:
        del ctx.backend.empty
      undo()
    assert sorted(model) == ['scores_per_label', 'scores_per_label_and_feature']
    scores = np.asarray(model['scores_per_label_and_feature'].glom())
    per_label = np.asarray(model['scores_per_label'].glom()).reshape(-1)
    assert scores.dtype == dt and scores.shape == (label_size, d) and per_label.dtype == dt and per_label.shape == (label_size,)
    if backend == 'hip':
      assert sorted(asked) == sorted([((n // workers, d), (n // workers, 1) if labels_2d else (n // workers,), label_size)]
                                     * workers)
    assert not [s for s in allocated if len(s) == 2 and s[0] >= n // workers and s[1] >= d], allocated   # no n x d tile
    _, bound = bounds(dt)
    for name, got, ref in (('wl', per_label, g['scores_per_label']), ('scores', scores, g['scores'])):
      share = nc._ratio(np.abs(np.asarray(got, np.float64) - ref), bound[name])
      print('naive_bayes %s %d workers %s: |%s - golden| is %.3g of the summed bounds (largest bound %.3g)'
            % (backend, workers, dt.name, name, share, bound[name].max()))
      assert share <= 1.0
    # the ten one-row queries and all 120 rows: exactly the recorded labels
    got = [int(nb.predict(model, sp.from_numpy(q.reshape(1, d).astype(dt)))) for q in queries]
    assert got == g['predicted'].tolist()
    assert int(nb.predict(model, queries[3].reshape(1, d))) == g['predicted'][3]       # a NumPy query of another dtype
    rows = nb.predict_labels(model, X)
    assert tuple(rows.shape) == (n,)
    rows = np.asarray(rows.glom())
    assert rows.dtype == np.int64 and rows.tobytes() == g['predicted_rows'].tobytes()
    return scores, per_label
  finally:
    sp.shutdown()


def check_df_and_integers(backend):
  """df is exact and the same at 1 and 4 workers; integer data takes the float64 path, bit for bit."""
  g = golden()
  data, labels, label_size, _ = nc.golden_input()
  n, d = data.shape
  from spartan_amd.examples import _nb
  seen = {}
  for workers in (1, 4):
    ctx = _start(backend, workers)
    try:
      step = _nb.nb_step
      dfs = []

      def watched(x, y, size, splits=0):
        out = step(x, y, size, splits=splits)
        dfs.append(np.asarray(ctx.backend.to_numpy(out[1])))
        return out
      _nb.nb_step = watched
      try:
        X = sp.from_numpy(data, tile_hint=(n // workers, d))
        model = nb.fit(X, sp.from_numpy(labels, tile_hint=(n // workers,)), label_size)
        ints = nb.fit(sp.from_numpy(data.astype(np.int32), tile_hint=(n // workers, d)),
                      sp.from_numpy(labels.astype(np.int32), tile_hint=(n // workers,)), label_size)
        f32 = nb.fit(sp.from_numpy(data.astype(np.int64), tile_hint=(n // workers, d)), labels.astype(np.uint8), label_size,
                     dtype=np.float32)
      finally:
        _nb.nb_step = step
      assert len(dfs) == 3 * workers and all(v.dtype == np.int64 for v in dfs)
      assert sum(dfs[:workers]).tobytes() == g['df'].tobytes() == sum(dfs[workers:2 * workers]).tobytes()
      a = np.asarray(model['scores_per_label_and_feature'].glom())
      b = np.asarray(ints['scores_per_label_and_feature'].glom())
      assert a.dtype == b.dtype == np.float64 and a.tobytes() == b.tobytes()
      assert np.asarray(f32['scores_per_label_and_feature'].glom()).dtype == np.float32
      seen[workers] = a
    finally:
      sp.shutdown()
  want, _ = bounds(np.dtype(np.float64))             # both runs are within the 'after' bound of the exact scores
  assert np.all(np.abs(seen[1] - seen[4]) <= 2 * nc.fit_bound(want, data.shape, ALPHA, np.float64, 'after')['scores'])


def check_refusals(backend):
  data, labels, label_size, _ = nc.golden_input()
  n, d = data.shape
  _start(backend, 4)
  try:
    X = sp.from_numpy(data, tile_hint=(n // 4, d))
    for wrong, row in ((-1, 77), (label_size, 31), (10 ** 12, 119)):
      lab = labels.copy()
      lab[row] = wrong
      lab[min(row + 5, n - 1)] = wrong          # the lowest row is the one that is named
      with pytest.raises(IndexError, match='row %d ' % row):
        nb.fit(X, sp.from_numpy(lab, tile_hint=(n // 4,)), label_size)
    for alpha in (0.0, -1.0, float('nan'), float('inf')):
      with pytest.raises(ValueError, match='alpha'):
        nb.fit(X, labels, label_size, alpha)
    for size in (0, 129):
      with pytest.raises(ValueError, match='label_size'):
        nb.fit(X, labels, size)
    with pytest.raises(ValueError, match=r'\(n, d\)'):
      nb.fit(data.reshape(-1), labels, label_size)
    for bad in (labels[:-1], labels.reshape(2, 60)):
      with pytest.raises(ValueError, match='labels of shape'):
        nb.fit(X, bad, label_size)
    with pytest.raises(TypeError, match='integers'):
      nb.fit(X, labels.astype(np.float64), label_size)
    with pytest.raises(TypeError, match='dtype'):
      nb.fit(X, labels, label_size, dtype=np.int32)
    model = nb.fit(X, labels, label_size)
    with pytest.raises(ValueError, match='features'):
      nb.predict(model, data[:1, :5])
    # a document without a term: its label's scores are NaN, the others' are numbers
    zero = data.copy()
    zero[50] = 0
    scores = np.asarray(nb.fit(sp.from_numpy(zero, tile_hint=(n // 4, d)), labels, label_size)
                        ['scores_per_label_and_feature'].glom())
    assert np.isnan(scores).all(axis=1).tolist() == [l == labels[50] for l in range(label_size)]
    assert np.isfinite(np.delete(scores, labels[50], axis=0)).all()
  finally:
    sp.shutdown()


def test_the_golden_holds_the_reference_run():
  g = golden()
  data, labels, label_size, queries = nc.golden_input()
  n, d = data.shape
  assert int(g['whole_fit']) == 1                      # scores and scores_per_label are the reference's whole fit
  assert np.all(data >= 0) and np.all((data != 0).any(axis=1))
  for b in range(4):
    assert set(labels[b * 30:(b + 1) * 30].tolist()) == set(range(label_size))
  assert g['df'].tobytes() == (data > 0).sum(axis=0).astype(np.int64).tobytes()
  assert g['rms'].tobytes() == np.sqrt(np.square(data).sum(axis=1) * 1.0 / d).tobytes()
  want, _ = bounds(np.dtype(np.float64))
  theirs = nc.fit_bound(want, data.shape, ALPHA, np.float64, 'inside')
  for name, key in (('W', 'W'), ('wl', 'scores_per_label'), ('scores', 'scores')):
    share = nc._ratio(np.abs(np.asarray(g[key], nc.LD) - want[name]), theirs[name])
    print('the reference against the oracle: %s at %.3g of its own bound' % (name, share))
    assert share <= 1.0
  for q, p in zip(queries, g['predicted']):
    v = np.sort(g['scores'].dot(q))
    assert (v[-1] - v[-2]) / abs(v[-1]) >= 1e-3 and p == np.argmax(g['scores'].dot(q))
  rows = np.sort(data.dot(g['scores'].T), axis=1)
  assert ((rows[:, -1] - rows[:, -2]) / np.abs(rows[:, -1])).min() >= 1e-3


@pytest.mark.parametrize('labels_2d', (True, False), ids=('labels_nx1', 'labels_n'))
@pytest.mark.parametrize('workers', (1, 3, 4))
def test_the_driver_reproduces_the_reference_cpu(workers, labels_2d):
  check_driver('numpy', workers, np.float64, labels_2d)


def test_float32_on_the_numpy_backend_finds_the_same_labels():
  check_driver('numpy', 4, np.float32)


def test_df_is_exact_and_integer_data_takes_the_float64_path_cpu():
  check_df_and_integers('numpy')


def test_refusals_cpu():
  check_refusals('numpy')
