"""sp_rowdot_link_colsum_f32 (csrc/rowdot.hip) on the device: every link against float64 NumPy within a derived
bound, determinism, `accumulate`, refused layouts, link 0 against the entry point it shares a kernel with, overflow
pinned to NumPy's float32, and the logistic gradients through the expression API and examples/logreg.py."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from spartan_amd import _hip, kernels  # noqa: E402
from spartan_amd import devarray as D  # noqa: E402

RNG = np.random.RandomState(20150709)
EPS = np.finfo(np.float32).eps
LINKS = (_hip.SP_LINK_IDENTITY, _hip.SP_LINK_EXP_RATIO, _hip.SP_LINK_SIGMOID)


def dev(a):
  return D.from_numpy(a)


def host(t):
  return t.numpy()


def _link64(t, link):
  if link == _hip.SP_LINK_EXP_RATIO:
    e = np.exp(t)
    return e / (e + 1)
  if link == _hip.SP_LINK_SIGMOID:
    return 1 / (1 + np.exp(-t))
  return t


def _want_and_bound(x, w, y, link):
  """float64 statement of the kernel and the bound on |got - want|.  The links are 1-Lipschitz with values in [0, 1]
  (the identity: |t| <= |x_i|.|w|), expf and the division are within 2 ulp, so the error of the fp32 row dot of d
  terms passes through the link unamplified, one more rounding each for the link, the subtraction and the product,
  and the column sum of n terms adds n more:
      |got - want|_c <= (n + d + 16) eps scale_c + 1e-30,   scale_c = sum_i |x_ic| (|x_i|.|w| + 1 + |y_i|)."""
  n, d = x.shape
  x64, w64 = x.astype(np.float64), w.astype(np.float64).reshape(d)
  r = _link64(x64.dot(w64), link)
  ya = 0.0
  if y is not None:
    r = r - y.reshape(n)
    ya = np.abs(y.astype(np.float64).reshape(n))
  want = (x64 * r[:, None]).sum(0)
  scale = (np.abs(x64) * (np.abs(x64).dot(np.abs(w64)) + 1 + ya)[:, None]).sum(0)
  return want, (n + d + 16) * EPS * scale + 1e-30


@pytest.mark.parametrize('n,d,pad', [(1000, 4096, 0), (257, 64, 0), (5, 260, 4), (3000, 4092, 8), (1, 4, 0), (70000, 512, 0)])
@pytest.mark.parametrize('with_y', [True, False])
@pytest.mark.parametrize('link', LINKS)
def test_rowdot_link_colsum_kernel(n, d, pad, with_y, link):
  x = (RNG.rand(n, d) - 0.5).astype(np.float32)           # |t| <= d / 4: far below expf's overflow at 88
  w = (RNG.rand(d) - 0.5).astype(np.float32)
  y = (RNG.rand(n) - 0.5).astype(np.float32) if with_y else None
  big = D.zeros((n, d + pad), np.float32)
  big[:, :d] = dev(x)
  xd = big[:, :d]
  out = D.full((d,), 3.0, np.float32)
  yd = dev(y) if with_y else None
  assert kernels.rowdot_link_colsum(xd, dev(w), yd, out, link) is True
  want, bound = _want_and_bound(x, w, y, link)
  got = host(out)
  err = np.abs(got - want)
  print('link %d n %d d %d y %d: max err / bound = %.3g' % (link, n, d, with_y, float(np.max(err / bound))))
  assert np.all(err <= bound)
  first = got.copy()
  assert kernels.rowdot_link_colsum(xd, dev(w), yd, out, link)
  np.testing.assert_array_equal(host(out), first)                              # identical bits on every run
  assert kernels.rowdot_link_colsum(xd, dev(w), yd, out, link, accumulate=True)
  np.testing.assert_array_equal(host(out), first + first)
  if link == _hip.SP_LINK_IDENTITY:
    # the entry point of the least-squares gradient is this link under its old name: the same bits
    old = D.full((d,), 5.0, np.float32)
    assert kernels.rowdot_colsum(xd, dev(w), yd, old)
    np.testing.assert_array_equal(host(old), first)
  # layouts the kernel does not take are reported, not guessed at
  if d > 4:
    assert kernels.rowdot_link_colsum(big[:, 1:d - 3], dev(w[:d - 4]), None, D.empty((d - 4,), np.float32), link) is False


def test_unknown_link_is_an_error():
  x, w, out = D.zeros((8, 16), np.float32), D.zeros((16,), np.float32), D.full((16,), 3.0, np.float32)
  for link in (3, -1, 7):
    with pytest.raises(Exception, match='unknown link'):
      kernels.rowdot_link_colsum(x, w, None, out, link)
  np.testing.assert_array_equal(host(out), np.full(16, 3.0, np.float32))       # nothing was launched
  import spartan_amd as sp
  ctx = sp.initialize('hip', num_workers=1)
  try:
    with pytest.raises(ValueError, match='unknown link'):
      ctx.backend.rowdot_link_colsum(x, np.zeros((16, 1), np.float32), None, 3)
  finally:
    sp.shutdown()


def _overflow_data(d=64):
  """One row with t = x . w near +100 and one near -100: clear of expf's float32 overflow threshold (88.7) whatever
  the order of the sum."""
  x = np.empty((2, d), np.float32)
  x[0] = 100.0 / d
  x[1] = -100.0 / d
  return x, np.ones(d, np.float32), np.array([0.25, 0.75], np.float32)


def test_overflow_is_numpys_float32():
  x, w, y = _overflow_data()
  one = np.float32(1)
  t32 = x.dot(w.reshape(-1, 1))
  assert t32.dtype == np.float32 and t32[0, 0] > 95 and t32[1, 0] < -95
  with np.errstate(over='ignore', invalid='ignore', under='ignore'):
    e = np.exp(t32)
    ratio32 = (x * (e / (e + one) - y.reshape(2, 1))).sum(0)
    sig32 = (x * (one / (one + np.exp(-t32)) - y.reshape(2, 1))).sum(0)
  assert np.all(np.isnan(ratio32)) and np.all(np.isfinite(sig32))              # what NumPy's float32 gives
  out = D.empty((64,), np.float32)
  assert kernels.rowdot_link_colsum(dev(x), dev(w), dev(y), out, _hip.SP_LINK_EXP_RATIO)
  assert np.all(np.isnan(host(out)))                                           # inf / inf in the +100 row, every column
  assert kernels.rowdot_link_colsum(dev(x), dev(w), dev(y), out, _hip.SP_LINK_SIGMOID)
  got = host(out)
  want, bound = _want_and_bound(x, w, y, _hip.SP_LINK_SIGMOID)
  assert np.all(np.isfinite(got))
  assert np.all(np.abs(got - sig32.astype(np.float64)) <= bound) and np.all(np.abs(got - want) <= bound)
  # through the expression API: the one-pass node and the two launches it replaces give the same NaN pattern
  import spartan_amd as sp
  from spartan_amd.expr.rowdot import RowDotColSumExpr
  optimize = importlib.import_module('spartan_amd.expr.optimize')
  sp.initialize('hip', num_workers=1)
  try:
    xv, yv = sp.Val(val=sp.from_numpy(x).force()), sp.Val(val=sp.from_numpy(y.reshape(2, 1)).force())
    wv = w.reshape(-1, 1)

    def ratio():
      g = sp.exp(sp.dot(xv, wv))
      return sp.sum(xv * (g / (g + 1) - yv), axis=0)

    def sigmoid():
      return sp.sum(xv * (1 / (1 + sp.exp(-sp.dot(xv, wv))) - yv), axis=0)
    for build in (ratio, sigmoid):
      one_pass = build().optimized()
      assert isinstance(one_pass, RowDotColSumExpr)
      a = one_pass.glom()
      optimize.FLAGS['opt_rowdot_fusion'] = False
      try:
        stated = build().optimized()
        assert not isinstance(stated, RowDotColSumExpr)
        b = stated.glom()
      finally:
        optimize.FLAGS['opt_rowdot_fusion'] = True
      np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
      assert np.all(np.isnan(a)) == (build is ratio) and np.any(np.isnan(a)) == (build is ratio)
  finally:
    sp.shutdown()


@pytest.mark.parametrize('workers', [1, 3, 8])
@pytest.mark.parametrize('n,d', [(17, 4), (1000, 4096), (5000, 132), (64, 260)])
def test_logistic_gradients_run_as_one_pass_per_tile(workers, n, d):
  """Both spellings through the expression API on 'hip', ragged row tilings, the smallest / largest widths: rewritten,
  one rowdot_link_colsum call per row tile, values within the kernel's bound."""
  import spartan_amd as sp
  from spartan_amd.expr.rowdot import RowDotColSumExpr
  ctx = sp.initialize('hip', num_workers=workers)
  try:
    rng = np.random.RandomState(n + d)
    xh, yh = (rng.rand(n, d) - 0.5).astype(np.float32), (rng.rand(n, 1) - 0.5).astype(np.float32)
    w = (rng.rand(d, 1) - 0.5).astype(np.float32)
    x, y = sp.Val(val=sp.from_numpy(xh).force()), sp.Val(val=sp.from_numpy(yh).force())

    def ratio():
      g = sp.exp(sp.dot(x, w))
      return g / (g + 1)

    def sigmoid():
      return 1 / (1 + sp.exp(-sp.dot(x, w)))
    calls = []
    inner = ctx.backend.rowdot_link_colsum
    ctx.backend.rowdot_link_colsum = lambda *a: (calls.append(a[3]), inner(*a))[1]
    try:
      for build, link, with_y in ((lambda: sp.sum(x * (ratio() - y), axis=0), _hip.SP_LINK_EXP_RATIO, True),
                                  (lambda: sp.sum((sigmoid() - y) * x, axis=0), _hip.SP_LINK_SIGMOID, True),
                                  (lambda: sp.sum(x * ratio(), axis=0), _hip.SP_LINK_EXP_RATIO, False),
                                  (lambda: sp.sum(x * sigmoid(), axis=0), _hip.SP_LINK_SIGMOID, False)):
        e = build().optimized()
        assert isinstance(e, RowDotColSumExpr) and e.link == link
        del calls[:]
        got = e.glom()
        assert calls == [link] * len(x.val.tiles)                              # one pass per row tile
        assert got.dtype == np.float32 and got.shape == (d,)
        want, bound = _want_and_bound(xh, w, yh if with_y else None, link)
        assert np.all(np.abs(got - want) <= bound)
    finally:
      del ctx.backend.rowdot_link_colsum
  finally:
    sp.shutdown()


def test_logreg_fit_one_pass_equals_the_stated_launches():
  """examples.logreg: ten steps through the rewrite against ten steps with the rewrite off (fp32 sums in two
  different orders) and against the reference's train() in float64 NumPy."""
  import spartan_amd as sp
  from spartan_amd.examples import logreg
  optimize = importlib.import_module('spartan_amd.expr.optimize')
  ctx = sp.initialize('hip', num_workers=3)
  try:
    rng = np.random.RandomState(4)
    xh, yh = (rng.rand(3001, 256) - 0.5).astype(np.float32), rng.rand(3001, 1).astype(np.float32)
    w = (rng.rand(256, 1) - 0.5).astype(np.float32)
    x, y = sp.Val(val=sp.from_numpy(xh).force()), sp.Val(val=sp.from_numpy(yh).force())
    calls = []
    inner = ctx.backend.rowdot_link_colsum
    ctx.backend.rowdot_link_colsum = lambda *a: (calls.append(a[3]), inner(*a))[1]
    try:
      w1 = logreg.fit(x, y, 10, alpha=1e-5, w=w)
      assert calls == [_hip.SP_LINK_EXP_RATIO] * (10 * len(x.val.tiles))
      optimize.FLAGS['opt_rowdot_fusion'] = False
      try:
        w0 = logreg.fit(x, y, 10, alpha=1e-5, w=w)
      finally:
        optimize.FLAGS['opt_rowdot_fusion'] = True
      assert len(calls) == 10 * len(x.val.tiles)
    finally:
      del ctx.backend.rowdot_link_colsum
    np.testing.assert_allclose(w1, w0, rtol=1e-5, atol=2e-6)
    x64, ww = xh.astype(np.float64), w.astype(np.float64)
    for _ in range(10):
      g = np.exp(x64.dot(ww))
      ww = ww - (x64 * (g / (g + 1) - yh)).sum(0).reshape((256, 1)) * 1e-5
    np.testing.assert_allclose(w1, ww, rtol=1e-4, atol=2e-6)
  finally:
    sp.shutdown()


def test_backend_falls_back_to_the_stated_launches_for_a_refused_layout():
  """HipBackend.rowdot_link_colsum on a tile the kernel does not take (rows not 16-byte aligned): the dot, the link
  with the backend's own ops and the map -> column sum, same values."""
  import spartan_amd as sp
  ctx = sp.initialize('hip', num_workers=1)
  try:
    n, d = 300, 64
    x = (RNG.rand(n, d + 3) - 0.5).astype(np.float32)
    w = (RNG.rand(d, 1) - 0.5).astype(np.float32)
    y = RNG.rand(n, 1).astype(np.float32)
    xd = dev(x)[:, 1:d + 1]
    assert kernels.rowdot_link_colsum(xd, dev(w.reshape(d)), None, D.empty((d,), np.float32), 1) is False
    for link in LINKS:
      got = host(ctx.backend.rowdot_link_colsum(xd, w, dev(y), link))
      want, bound = _want_and_bound(x[:, 1:d + 1], w, y, link)
      assert got.dtype == np.float32 and np.all(np.abs(got - want) <= bound)
  finally:
    sp.shutdown()


def test_two_ranks_hip_shared_gpu():
  """Two ranks with the HIP backend sharing GPU 0 (tests/mp_logreg_worker.py): every rank's row tiles contribute a
  (d,) partial, the combined gradient equals the single-process one."""
  from tests.test_multiprocess import _run_ranks
  _run_ranks(2, 'mp_logreg_worker.py', ['4', 'hip'])
