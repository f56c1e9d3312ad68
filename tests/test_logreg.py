"""The one-pass rewrite of the logistic gradients (optimize.RowDotColSumFusion with a link, expr/rowdot.py,
examples/logreg.py): which DAGs it takes and with which link, that a backend without `rowdot_link_colsum` is never
handed one, that everything else stays as stated, and that the plan cache keeps the links apart -- host logic on the
NumPy oracle backend with stand-ins for the kernel; the kernel itself is tested on the GPU (test_logreg_gpu.py)."""
import importlib

import numpy as np
import pytest

import spartan_amd as sp
from oracle.np_backend import NumpyBackend
from spartan_amd.examples import logreg, lreg
from spartan_amd.expr import rowdot
from spartan_amd.expr.rowdot import LINK_EXP_RATIO, LINK_IDENTITY, LINK_SIGMOID, RowDotColSumExpr

optimize = importlib.import_module('spartan_amd.expr.optimize')     # (the package attribute is the function)


class _WithKernel(NumpyBackend):
  """The oracle backend plus a NumPy statement of sp_rowdot_colsum_f32 only (tests/test_rowdot.py's stand-in)."""
  calls = 0

  def rowdot_colsum(self, x, w, y):
    type(self).calls += 1
    t = x.astype(np.float32).dot(np.asarray(w, np.float32).reshape(-1, 1))
    r = t if y is None else t - np.asarray(y).reshape(t.shape)
    return (x * r).sum(0).astype(np.float32)


class _WithLinkKernel(_WithKernel):
  """... plus a NumPy float32 statement of sp_rowdot_link_colsum_f32."""
  link_calls = []

  def rowdot_link_colsum(self, x, w, y, link):
    type(self).link_calls.append(link)
    one = np.float32(1)
    t = x.astype(np.float32).dot(np.asarray(w, np.float32).reshape(-1, 1))
    if link == LINK_EXP_RATIO:
      e = np.exp(t)
      t = e / (e + one)
    elif link == LINK_SIGMOID:
      t = one / (one + np.exp(-t))
    else:
      assert link == LINK_IDENTITY, link
    r = t if y is None else t - np.asarray(y).reshape(t.shape)
    return (x * r).sum(0).astype(np.float32)


def _data(n=203, d=64, seed=0):
  rng = np.random.RandomState(seed)
  return (rng.rand(n, d) - 0.5).astype(np.float32), rng.rand(n, 1).astype(np.float32), (rng.rand(d, 1) - 0.5).astype(np.float32)


def _sigmoid64(xh, w):
  g = np.exp(xh.astype(np.float64).dot(w.astype(np.float64)))
  return g / (g + 1)


def _spellings(x, y, w):
  """(name, builder, link, uses y): both spellings, with and without `- y`, x on either side of the product."""
  def ratio():
    g = sp.exp(sp.dot(x, w))
    return g / (g + 1)

  def ratio_swapped():
    g = sp.exp(sp.dot(x, w))
    return g / (1 + g)

  def sigmoid():
    return 1 / (1 + sp.exp(-sp.dot(x, w)))

  def sigmoid_swapped():
    return 1.0 / (sp.exp(sp.negative(sp.dot(x, w))) + 1.0)

  out = []
  for name, L, link in (('ratio', ratio, LINK_EXP_RATIO), ('ratio_swapped', ratio_swapped, LINK_EXP_RATIO),
                        ('sigmoid', sigmoid, LINK_SIGMOID), ('sigmoid_swapped', sigmoid_swapped, LINK_SIGMOID)):
    out.append((name + ': x * (L - y)', lambda L=L: sp.sum(x * (L() - y), axis=0), link, True))
    out.append((name + ': (L - y) * x', lambda L=L: sp.sum((L() - y) * x, axis=0), link, True))
    out.append((name + ': x * L', lambda L=L: sp.sum(x * L(), axis=0), link, False))
    out.append((name + ': L * x', lambda L=L: sp.sum(L() * x, axis=0), link, False))
  return out


@pytest.mark.parametrize('workers', [1, 4])
def test_logistic_dags_are_rewritten_with_their_link(workers):
  xh, yh, w = _data()
  yp = _sigmoid64(xh, w)
  x64 = xh.astype(np.float64)
  sp.initialize(backend=_WithLinkKernel(), num_workers=workers)
  try:
    x, y = sp.Val(val=sp.from_numpy(xh).force()), sp.Val(val=sp.from_numpy(yh).force())
    g = logreg.gradient(x, y, w).optimized()                       # the reference's spelling, through the driver
    assert isinstance(g, RowDotColSumExpr) and g.link == LINK_EXP_RATIO
    assert 'exp_ratio' in g.pretty_str()
    for name, build, link, with_y in _spellings(x, y, w):
      e = build().optimized()
      assert isinstance(e, RowDotColSumExpr), name
      assert e.link == link, name
      assert rowdot.LINK_NAMES[link] in e.pretty_str()
      _WithLinkKernel.link_calls, _WithKernel.calls = [], 0
      got = e.glom()
      assert got.shape == (64,) and got.dtype == np.float32, name
      assert _WithLinkKernel.link_calls == [link] * len(x.val.tiles), name       # one call per row tile
      assert _WithKernel.calls == 0, name
      want = (x64 * (yp - yh if with_y else yp)).sum(0)
      np.testing.assert_allclose(got, want, rtol=2e-5, err_msg=name)
  finally:
    sp.shutdown()


def test_link_values_are_the_headers():
  from spartan_amd import _hip
  assert (LINK_IDENTITY, LINK_EXP_RATIO, LINK_SIGMOID) == (_hip.SP_LINK_IDENTITY, _hip.SP_LINK_EXP_RATIO, _hip.SP_LINK_SIGMOID) == (0, 1, 2)
  assert RowDotColSumExpr(x=None, y=None, w=None, tile_hint=None).link == LINK_IDENTITY     # the default


def test_backend_with_the_identity_kernel_only_keeps_logistic_dags_as_stated():
  xh, yh, w = _data()
  sp.initialize(backend=_WithKernel(), num_workers=2)
  try:
    x, y = sp.Val(val=sp.from_numpy(xh).force()), sp.Val(val=sp.from_numpy(yh).force())
    g = lreg.gradient(x, y, w).optimized()
    assert isinstance(g, RowDotColSumExpr) and g.link == LINK_IDENTITY
    for name, build, link, with_y in _spellings(x, y, w):
      assert not isinstance(build().optimized(), RowDotColSumExpr), name
    got = logreg.gradient(x, y, w).optimized().glom()
    np.testing.assert_allclose(got, (xh.astype(np.float64) * (_sigmoid64(xh, w) - yh)).sum(0), rtol=2e-5)
  finally:
    sp.shutdown()
  sp.initialize(backend=NumpyBackend(), num_workers=2)
  try:
    x, y = sp.Val(val=sp.from_numpy(xh).force()), sp.Val(val=sp.from_numpy(yh).force())
    assert not isinstance(lreg.gradient(x, y, w).optimized(), RowDotColSumExpr)
    assert not isinstance(logreg.gradient(x, y, w).optimized(), RowDotColSumExpr)
  finally:
    sp.shutdown()


def test_rewrite_leaves_everything_else_alone():
  xh, yh, w = _data(d=64)
  w2 = w[::-1].copy()
  sp.initialize(backend=_WithLinkKernel(), num_workers=2)
  try:
    x, y = sp.Val(val=sp.from_numpy(xh).force()), sp.Val(val=sp.from_numpy(yh).force())
    t = sp.dot(x, w)
    g, h = sp.exp(t), sp.exp(sp.dot(x, w2))
    g64 = sp.exp(sp.dot(x, w.astype(np.float64)))
    xc = sp.Val(val=sp.from_numpy(xh, tile_hint=(203, 16)).force())
    gc = sp.exp(sp.dot(xc, w))
    x6 = sp.Val(val=sp.from_numpy(xh[:, :62].copy()).force())
    g6 = sp.exp(sp.dot(x6, w[:62]))
    g2t = sp.exp(2 * t)
    keep = [
        sp.sum(x * (g / (g + 2) - y), axis=0),                     # another constant than 1
        sp.sum(x * (g / (h + 1) - y), axis=0),                     # two different dots
        sp.sum(x * (g2t / (g2t + 1) - y), axis=0),                 # exp of something that is not the dot
        sp.sum(x * (sp.map(t, fn=np.tanh) - y), axis=0),            # another link: tanh(t)
        sp.sum(x * (g / (g + 1) - y), axis=1),                     # row sums
        sp.max(x * (g / (g + 1) - y), axis=0),                     # not a sum
        sp.sum(x * (g64 / (g64 + 1) - y), axis=0),                 # a float64 weight vector
        sp.sum(xc * (gc / (gc + 1) - y), axis=0),                  # x tiled by columns
        sp.sum(x6 * (g6 / (g6 + 1) - y), axis=0),                  # 62 columns: not a multiple of 4
        sp.sum(x * (1 / (2 + sp.exp(-t)) - y), axis=0),            # the second spelling with another constant
        sp.sum(x * (1 / (1 + sp.exp(t)) - y), axis=0),             # ... without the negation
    ]
    _WithLinkKernel.link_calls = []
    for e in keep:
      assert not isinstance(e.optimized(), RowDotColSumExpr), e
    x64 = xh.astype(np.float64)
    e64 = np.exp(x64.dot(w.astype(np.float64)))
    np.testing.assert_allclose(keep[0].glom(), (x64 * (e64 / (e64 + 2) - yh)).sum(0), rtol=2e-5)
    np.testing.assert_allclose(keep[4].glom(), (x64 * (e64 / (e64 + 1) - yh)).sum(1), rtol=2e-5, atol=1e-6)
    assert _WithLinkKernel.link_calls == []
    # the flag that turns the least-squares rewrite off turns these off too
    optimize.FLAGS['opt_rowdot_fusion'] = False
    try:
      assert not isinstance(logreg.gradient(x, y, w).optimized(), RowDotColSumExpr)
    finally:
      optimize.FLAGS['opt_rowdot_fusion'] = True
    assert isinstance(logreg.gradient(x, y, w).optimized(), RowDotColSumExpr)
  finally:
    sp.shutdown()


def test_fit_through_the_rewrite_equals_the_fit_without_it_and_numpy():
  xh, yh, w = _data()
  sp.initialize(backend=_WithLinkKernel(), num_workers=4)
  try:
    x, y = sp.Val(val=sp.from_numpy(xh).force()), sp.Val(val=sp.from_numpy(yh).force())
    _WithLinkKernel.link_calls = []
    w1 = logreg.fit(x, y, 5, alpha=1e-3, w=w)
    assert _WithLinkKernel.link_calls == [LINK_EXP_RATIO] * (5 * len(x.val.tiles))
    optimize.FLAGS['opt_rowdot_fusion'] = False
    try:
      w0 = logreg.fit(x, y, 5, alpha=1e-3, w=w)
    finally:
      optimize.FLAGS['opt_rowdot_fusion'] = True
    assert len(_WithLinkKernel.link_calls) == 5 * len(x.val.tiles)            # none with the rewrite off
    np.testing.assert_allclose(w1, w0, rtol=1e-5, atol=1e-6)
    # the reference's train() (sgd.py:34-39 over logistic_regression.py:15-17) in float64 NumPy
    x64, ww = xh.astype(np.float64), w.astype(np.float64)
    for _ in range(5):
      g = np.exp(x64.dot(ww))
      grad = (x64 * (g / (g + 1) - yh)).sum(0).reshape((64, 1))
      ww = ww - grad * 1e-3
    np.testing.assert_allclose(w1, ww, rtol=1e-4)
    assert w1.shape == (64, 1)
  finally:
    sp.shutdown()


@pytest.mark.parametrize('logistic_first', [False, True])
def test_plan_cache_keeps_the_links_apart(logistic_first):
  """DAGs of the same shapes that differ only in the link never share a recorded recipe, in either order -- and a
  second round is answered from the plan table with the same links."""
  from spartan_amd.expr import plan
  xh, yh, w = _data()
  sp.initialize(backend=_WithLinkKernel(), num_workers=2)
  try:
    plan.clear()
    x, y = sp.Val(val=sp.from_numpy(xh).force()), sp.Val(val=sp.from_numpy(yh).force())
    builders = [(lambda: lreg.gradient(x, y, w), LINK_IDENTITY), (lambda: logreg.gradient(x, y, w), LINK_EXP_RATIO),
                (lambda: sp.sum(x * (1 / (1 + sp.exp(-sp.dot(x, w))) - y), axis=0), LINK_SIGMOID)]
    if logistic_first:
      builders = builders[::-1]
    for round_ in range(2):
      hits = plan.stats['hits']
      for build, link in builders:
        e = build().optimized()
        assert isinstance(e, RowDotColSumExpr) and e.link == link, (round_, link)
      if round_:
        assert plan.stats['hits'] == hits + len(builders)
    x64 = xh.astype(np.float64)
    np.testing.assert_allclose(logreg.gradient(x, y, w).optimized().glom(), (x64 * (_sigmoid64(xh, w) - yh)).sum(0), rtol=2e-5)
    np.testing.assert_allclose(lreg.gradient(x, y, w).optimized().glom(), (x64 * (x64.dot(w.astype(np.float64)) - yh)).sum(0), rtol=2e-5)
  finally:
    sp.shutdown()


def test_two_socket_ranks():
  """Every rank's row tiles contribute a (d,) partial; the combined gradient equals the single-process one
  (tests/mp_logreg_worker.py)."""
  from tests.test_multiprocess import _run_ranks
  _run_ranks(2, 'mp_logreg_worker.py', ['4'])
