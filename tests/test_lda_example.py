"""examples/lda: the LDA (CVB0) driver.  CPU leg: the host framework on the injected NumPy backend, where the tile body
is the NumPy restatement beside the driver (examples/_lda.py).  The GPU leg (tests/test_lda_gpu.py) runs check_driver
of this file on the HIP backend (sp_lda_step).

Input: tests/lda_cases.golden_input -- 48 terms x 40 documents of small counts, document 7 empty, term 11 in no
document, k = 5 fixed starting counts.  Yardstick: tests/golden/lda_w4.npz, recorded by tests/golden/make_golden_lda.py
from the reference's own mappers (on the whole matrix and on the four bands of 10 documents, max_iter_per_doc 1 and 2)
and from its whole learn_topics at 4 workers (max_iter = 2), which that script found equal to 4 . N + the sum of the
four bands' deltas per iteration: every document tile adds its own copy of the counts.  The driver keeps that, so it is
run with four tiles of 10 documents whatever the number of workers, and once with one tile to show the difference.

The reference computes in float64 in another association than the tile body, so both carry rounding errors against the
exact result: the tolerance per entry is the derived bound of tests/lda_cases (eps for one step, driver_eps for the
whole run) for the dtype under test plus the same bound for float64, relative to the recorded value; the share that is
used is printed."""
import functools
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd.examples import _lda
from spartan_amd.examples.lda import learn_topics
from tests import lda_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
V, D, K, BANDS = lc.GOLDEN_V, lc.GOLDEN_D, lc.GOLDEN_K, lc.GOLDEN_BANDS
ALPHA, ETA = 0.1, 0.1


@functools.lru_cache(maxsize=None)
def golden():
  g = dict(np.load(os.path.join(HERE, 'golden', 'lda_w4.npz')))
  x, n0 = lc.golden_input()
  assert g['x'].tobytes() == x.tobytes() and g['n0'].tobytes() == n0.tobytes()
  for a in g.values():
    a.setflags(write=False)
  return g


def _start(backend, workers):
  if backend == 'hip':
    return sp.initialize('hip', num_workers=workers)
  from oracle.np_backend import NumpyBackend
  return sp.initialize(backend=NumpyBackend(), num_workers=workers)


def _close(got, want, tol, what, floor=0.0):
  """|got - want| <= tol |want| + floor entry by entry, NaNs in the same places, an exact 0 where the limit is 0; prints
  the share of the limit that is used."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  nan = np.isnan(want)
  assert np.array_equal(np.isnan(got), nan), what
  err = np.abs(got - want)[~nan]
  lim = (tol * np.abs(want) + floor)[~nan]
  assert not np.any(err[lim == 0]), what
  share = float((err[lim > 0] / lim[lim > 0]).max())
  print('%s: %.3g of the tolerance %.3g' % (what, share, tol))
  assert share <= 1.0, what


def check_tile_body(backend, dtype):
  """The tile body against every recorded output of the reference's two mappers."""
  g = golden()
  dt = np.dtype(dtype)
  ctx = _start(backend, 1)
  try:
    be = ctx.backend
    x, n0 = g['x'].astype(dt), g['n0'].astype(dt)
    pieces = [('whole', 0, D)] + [('band%d' % b, b * D // BANDS, (b + 1) * D // BANDS) for b in range(BANDS)]
    for p in (1, 2):
      for name, lo, hi in pieces:
        tol = {key: val + lc.eps(V, hi - lo, K, p, np.float64)[key] for key, val in lc.eps(V, hi - lo, K, p, dt).items()}
        xt, nt = be.from_numpy(np.ascontiguousarray(x[:, lo:hi])), be.from_numpy(n0)
        delta, doc_topics = _lda.lda_step(xt, nt, ALPHA, ETA, p)
        delta, doc_topics = np.asarray(be.to_numpy(delta)), np.asarray(be.to_numpy(doc_topics))
        assert delta.dtype == dt and doc_topics.dtype == dt
        want_delta = g['train_%s_p%d' % (name, p)] - g['n0']
        assert not np.any(delta[:, 11]) and not np.any(want_delta[:, 11])
        # (the recorded N + delta lost delta's low bits to N, and so did the subtraction: eps |N + delta| of float64)
        lost = np.where(want_delta != 0, np.finfo(np.float64).eps * g['train_%s_p%d' % (name, p)], 0.0)
        _close(delta, want_delta, tol['delta'], '%s %s delta %s p=%d' % (backend, dt.name, name, p), floor=lost)
        _close(doc_topics, g['doc_%s_p%d' % (name, p)], tol['doc_topics'], '%s %s doc_topics %s p=%d' % (backend, dt.name, name, p))
        only_delta = _lda.lda_step(xt, nt, ALPHA, ETA, p, want_doc_topics=False)
        only_topics = _lda.lda_step(xt, nt, ALPHA, ETA, p, want_delta=False)
        assert only_delta[1] is None and only_topics[0] is None
        assert np.asarray(be.to_numpy(only_delta[0])).tobytes() == delta.tobytes()
        assert np.asarray(be.to_numpy(only_topics[1])).tobytes() == doc_topics.tobytes()
  finally:
    sp.shutdown()


def check_driver(backend, workers, dtype, as_integers=False):
  """learn_topics on four tiles of 10 documents against the reference's whole run at 4 workers."""
  g = golden()
  dt = np.dtype(dtype)
  ctx = _start(backend, workers)
  try:
    x = g['x'].astype(np.int64 if as_integers else dt)
    X = sp.from_numpy(x, tile_hint=(V, D // BANDS))
    asked = []
    step = getattr(ctx.backend, 'lda_step', None)
    if step is not None:                       # watch what the driver asks of the kernel
      def watched(xx, nn, alpha, eta, iters, want_delta=True, want_doc_topics=True, splits=0):
        asked.append((tuple(xx.shape), bool(want_delta), bool(want_doc_topics)))
        return step(xx, nn, alpha, eta, iters, want_delta=want_delta, want_doc_topics=want_doc_topics, splits=splits)
      ctx.backend.lda_step = watched
    try:
      doc_topics, counts = learn_topics(X, K, alpha=ALPHA, eta=ETA, max_iter=2, max_iter_per_doc=1,
                                        topic_term_counts=np.array(g['n0']), dtype=None if as_integers else dt)
      assert tuple(doc_topics.shape) == (D, K) and tuple(counts.shape) == (K, V)
      doc_topics, counts = np.asarray(doc_topics.glom()), np.asarray(counts.glom())
    finally:
      if step is not None:
        del ctx.backend.lda_step
    assert doc_topics.dtype == dt and counts.dtype == dt
    tol = {key: val + lc.driver_eps(V, D // BANDS, K, 1, 2, BANDS, np.float64)[key]
           for key, val in lc.driver_eps(V, D // BANDS, K, 1, 2, BANDS, dt).items()}
    tag = '%s %d workers %s%s' % (backend, workers, dt.name, ' from int64' if as_integers else '')
    for name in ('w4_', 'chain_'):
      want_topics, want_counts = g[name + 'doc_topics'], g[name + ('counts' if name == 'w4_' else 'counts_normalised')]
      _close(doc_topics, want_topics, tol['doc_topics'], 'learn_topics %s doc_topics against %s' % (tag, name))
      _close(counts, want_counts, tol['counts'], 'learn_topics %s counts against %s' % (tag, name))
    assert np.all(np.isnan(doc_topics[7])) and np.all(np.abs(np.abs(counts).sum(axis=1) - 1) <= 4 * V * np.finfo(dt).eps)
    if step is not None:
      band = (V, D // BANDS)
      assert sorted(asked) == sorted([(band, True, False)] * (2 * BANDS) + [(band, False, True)] * BANDS)
    return doc_topics, counts
  finally:
    sp.shutdown()


@pytest.mark.parametrize('dtype', (np.float64, np.float32), ids=lambda d: np.dtype(d).name)
def test_the_tile_body_equals_the_reference_mappers(dtype):
  check_tile_body('numpy', dtype)


@pytest.mark.parametrize('workers', (1, 4))
def test_the_driver_equals_the_reference_run(workers):
  check_driver('numpy', workers, np.float64)


def test_a_float32_run_is_inside_the_two_iteration_bound():
  check_driver('numpy', 4, np.float32)


def test_integer_counts_run_in_float64():
  got = check_driver('numpy', 4, np.float64, as_integers=True)
  want = check_driver('numpy', 4, np.float64)
  assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


def test_one_tile_keeps_one_copy_of_the_counts():
  """With one tile of documents an iteration is N + delta: the reference's whole-matrix mapper, normalised."""
  g = golden()
  _start('numpy', 1)
  try:
    doc_topics, counts = learn_topics(sp.from_numpy(np.array(g['x']), tile_hint=(V, D)), K, alpha=ALPHA, eta=ETA,
                                      max_iter=1, max_iter_per_doc=2, topic_term_counts=sp.from_numpy(np.array(g['n0'])))
    n1 = g['train_whole_p2']
    tol = 2 * lc.driver_eps(V, D, K, 2, 1, 1, np.float64)['counts']
    _close(counts.glom(), n1 / np.abs(n1).sum(axis=1)[:, None], tol, 'one tile: counts')
    four = 4 * g['n0'] + sum(g['train_band%d_p2' % b] - g['n0'] for b in range(BANDS))
    assert np.abs(counts.glom() - four / np.abs(four).sum(axis=1)[:, None]).max() > 1e-4       # (not the four-tile result)
    assert tuple(doc_topics.shape) == (D, K) and np.all(np.isnan(doc_topics.glom()[7]))
    # no training at all: the inference on the start, the start normalised
    doc_topics, counts = learn_topics(np.array(g['x']), K, alpha=ALPHA, eta=ETA, max_iter=0, max_iter_per_doc=1,
                                      topic_term_counts=np.array(g['n0']))
    _close(doc_topics.glom(), g['doc_whole_p1'], 2 * lc.eps(V, D, K, 1, np.float64)['doc_topics'], 'max_iter = 0: doc_topics')
    _close(counts.glom(), g['n0'] / g['n0'].sum(axis=1)[:, None], 1e-14, 'max_iter = 0: counts')
    # the default start is the reference's expr.rand
    doc_topics, counts = learn_topics(np.array(g['x']), 3, max_iter=1)
    doc_topics, counts = doc_topics.glom(), counts.glom()
    assert doc_topics.shape == (D, 3) and counts.shape == (3, V) and counts.dtype == np.float64
    assert np.all(np.abs(np.delete(doc_topics, 7, axis=0).sum(axis=1) - 1) < 1e-12) and np.all(counts > 0)
  finally:
    sp.shutdown()


def test_refusals():
  g = golden()
  _start('numpy', 1)
  try:
    x, n0 = np.array(g['x']), np.array(g['n0'])
    for kw, match in ((dict(k_topics=0), 'k = 0'), (dict(k_topics=129), 'k = 129'), (dict(max_iter=-1), 'max_iter'),
                      (dict(max_iter_per_doc=0), 'iters = 0'), (dict(alpha=0.0), 'alpha'), (dict(eta=-1.0), 'eta'),
                      (dict(alpha=float('nan')), 'alpha'), (dict(eta=float('inf')), 'eta')):
      args = dict(k_topics=K, alpha=ALPHA, eta=ETA, max_iter=1, max_iter_per_doc=1)
      args.update(kw)
      with pytest.raises(ValueError, match=match):
        learn_topics(x, **args)
    with pytest.raises(ValueError, match='terms x documents'):
      learn_topics(x.reshape(-1), K)
    with pytest.raises(ValueError, match='topic_term_counts of shape'):
      learn_topics(x, K, topic_term_counts=n0[:, :-1])
    with pytest.raises(TypeError, match='float32 float64'):
      learn_topics(x, K, dtype=np.float16)
    # the tile body on host tiles
    with pytest.raises(TypeError, match='astype'):
      _lda.lda_step(x.astype(np.int32), n0, ALPHA, ETA, 1)
    with pytest.raises(TypeError, match='astype'):
      _lda.lda_step(x.astype(np.float32), n0, ALPHA, ETA, 1)
    with pytest.raises(ValueError, match='do not fit'):
      _lda.lda_step(x[:-1], n0, ALPHA, ETA, 1)
    with pytest.raises(ValueError, match='k = 129'):
      _lda.lda_step(x, np.ones((129, V)), ALPHA, ETA, 1)
    with pytest.raises(ValueError, match='iters = 0'):
      _lda.lda_step(x, n0, ALPHA, ETA, 0)
  finally:
    sp.shutdown()
