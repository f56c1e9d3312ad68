"""The NumPy restatement of the dual coordinate ascent pass (examples/_svm.dca_numpy) against the stated order of
tests/svm_cases.py byte for byte, the reference's recorded special rows, chain independence, the accuracy rule on the
golden input in both dtypes, the refusals of the shared check, and that header, binding and library name the same
function and the same limit.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, tile_checks
from spartan_amd.examples import _svm
from tests import svm_cases as sc

DTYPES = (np.float32, np.float64)
dtype_ids = dict(ids=lambda d: np.dtype(d).name)
# (m, d, chains): every m and d of the device tests once, the chains on both sides of m
SHAPES = ([(m, 3, c) for m in sc.MS for c in (1, 3)] + [(65, d, 2) for d in sc.DS]
          + [(7, 130, 7), (7, 65, 10), (200, 64, 7), sc.BIG_D + (2,)])


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d-%d' % s)
def test_the_numpy_body_is_the_stated_order_byte_for_byte(shape, dtype):
  m, d, chains = shape
  x, y, alpha, w0, s = sc.case(m, d, dtype)
  before = [a.copy() for a in (x, y, alpha, w0)]
  got_a, got_w = _svm.dca_numpy(x, y, alpha, w0, s, chains)
  want_a, want_w = sc.restated(x, y, alpha, w0, s, chains)
  assert got_a.shape == (m, 1) and got_w.shape == (chains, d) and got_a.dtype == got_w.dtype == np.dtype(dtype)
  assert got_a.reshape(m).tobytes() == want_a.tobytes() and got_w.tobytes() == want_w.tobytes()
  assert all(a.tobytes() == b.tobytes() for a, b in zip((x, y, alpha, w0), before))       # no operand is written
  if m:
    assert got_a.reshape(m).tobytes() != alpha.tobytes()
  for c, (lo, hi) in enumerate(sc.chain_rows(m, chains)):
    if lo == hi:
      assert got_w[c].tobytes() == w0.tobytes()          # a chain without rows: w0


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_lane_dot_is_the_stated_dot(dtype):
  rng = np.random.RandomState(3)
  for d in (1, 63, 64, 65, 130, 1000):
    p, r = rng.randn(d).astype(dtype), rng.randn(d).astype(dtype)
    pad = -(-d // 64) * 64
    pp, rp = np.zeros(pad, dtype), np.zeros(pad, dtype)
    pp[:d], rp[:d] = p, r
    assert _svm.lane_dot(pp, rp).tobytes() == sc.stated_dot(p, r).tobytes()


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_special_rows(dtype):
  """The reference's own _svm_disdca_train on the special rows (golden: float64).  By value: the reference adds the 7
  products of a row in NumPy's order, ours in the stated one, so the two differ by roundings -- 12 steps whose every
  quantity is of order 1 and whose gain (1 / (s q), s = 1.67, q near 1) is of order 1 leave less than 12 * 7 * 4 u,
  taken as 2^-40 in float64 (u = 2^-53) and 2^-11 in float32; a wrong branch of the clamp moves alpha by more than
  0.1.  NaN by position."""
  dt = np.dtype(dtype)
  x, y, alpha, w0, s = sc.special_case(dt)
  got_a, got_w = _svm.dca_numpy(x, y, alpha, w0, s, 1)
  want_a, want_w = sc.restated(x, y, alpha, w0, s, 1)
  assert sc.same(got_a.reshape(-1), want_a) and sc.same(got_w, want_w)
  g = sc.golden()
  ref_a, ref_w = g['special_alpha'].reshape(-1), g['special_w'].reshape(-1)
  tol = 2.0 ** -40 if dt == np.float64 else 2.0 ** -11
  for got, ref in ((got_a.reshape(-1), ref_a), (got_w.reshape(-1), ref_w)):
    assert (np.isnan(got) == np.isnan(ref)).all()
    ok = ~np.isnan(ref)
    err = np.abs(got[ok].astype(np.float64) - ref[ok]).max()
    print('special rows %s: max abs distance to the reference %.3g (limit %.3g)' % (dt.name, err, tol))
    assert err <= tol
  # what the header says of them
  rows = sc.SPECIAL_ROWS
  nan_row = rows['NaN in x']
  assert np.isnan(got_w[0]).tolist() == np.isnan(x[nan_row]).tolist()         # dl is finite: exactly where x is NaN
  assert not np.isnan(got_a[:nan_row]).any() and got_a[nan_row, 0] == y[nan_row]          # NaN clamps to 1
  assert np.isfinite(got_a[nan_row + 1:]).all()                                # later rows keep running
  upto = lambda i: _svm.dca_numpy(x[:i], y[:i], alpha[:i], w0, s, 1)[1]   # noqa: E731
  for name in ('zero row', 'zero row with y = 0'):
    i = rows[name]
    assert upto(i + 1).tobytes() == upto(i).tobytes(), name                    # w unchanged
  assert got_a[rows['zero row with y = 0'], 0] == 0 and got_a[rows['y = 0'], 0] == 0      # y = 0: alpha' = 0 * c = 0


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_chains_are_independent(dtype):
  m, d = 65, 7
  x, y, alpha, w0, s = sc.case(m, d, dtype)
  for body in (_svm.dca_numpy, sc.restated):
    whole_a, whole_w = body(x, y, alpha, w0, s, 4)
    for c, (lo, hi) in enumerate(sc.chain_rows(m, 4)):
      a, w = body(x[lo:hi], y[lo:hi], alpha[lo:hi], w0, s, 1)
      assert np.asarray(whole_a).reshape(m)[lo:hi].tobytes() == np.asarray(a).reshape(-1).tobytes()
      assert whole_w[c].tobytes() == w[0].tobytes()
  assert sc.chain_rows(7, 10)[:3] == [(0, 0), (0, 1), (1, 2)] and sc.chain_rows(0, 3) == [(0, 0)] * 3


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_accuracy_against_the_reference(dtype):
  """The rule of tests/svm_cases.py on the golden input: the stated order (and the NumPy body, which is its bytes)
  within 8 e_ref of the yardstick (times 2^29 in float32)."""
  x, y = sc.golden_input()
  g = sc.golden()
  assert g['data'].tobytes() == x.tobytes() and g['labels'].tobytes() == y.tobytes() and int(g['whole_run']) == 1
  alphas, w = sc.run(sc.restated, x, y, dtype=dtype)
  alphas2, w2 = sc.run(_svm.dca_numpy, x, y, dtype=dtype)
  assert all(a.tobytes() == b.tobytes() for a, b in zip(alphas, alphas2)) and w.tobytes() == w2.tobytes()
  sc.check_accuracy({'alpha_1': alphas[0], 'alpha_3': alphas[-1], 'w_3': w}, dtype, 'restated')
  # the training accuracy the yardstick's w gives (recorded, not a constant)
  want = sc.golden_yardstick(dtype)['w_3']
  acc = lambda wv: float((np.where(np.asarray(x, sc.LD).dot(np.asarray(wv, sc.LD)) >= 0, 1, -1) == y.reshape(-1)).mean())  # noqa: E731
  print('training accuracy after %d iterations: yardstick %.3f, restated %s %.3f' % (sc.ITERS, acc(want), np.dtype(dtype).name, acc(w)))
  assert acc(w) == acc(want)


def test_refusals_and_absent_tiles():
  from oracle.np_backend import NumpyBackend
  from spartan_amd.array import distarray
  f32 = np.dtype(np.float32)
  x, y, alpha, w0, s = sc.case(9, 3, f32)

  def both(exc, match, xx=x, yy=y, aa=alpha, ww=w0, ss=s, chains=1):
    """The check and the NumPy body refuse alike."""
    operands = (xx, yy, aa, ww)
    with pytest.raises(exc, match=match):
      tile_checks.check_svm_dca([t.dtype for t in operands], [t.shape for t in operands], ss, chains)
    with pytest.raises(exc, match=match):
      _svm.svm_dca(xx, yy, aa, ww, ss, chains=chains)

  sp.initialize(backend=NumpyBackend(), num_workers=1)
  try:
    out = _svm.svm_dca(x, y.reshape(9, 1), alpha, w0.reshape(3, 1), s, chains=2)
    assert out.shape == (9, 1) and out.tobytes() == _svm.dca_numpy(x, y, alpha, w0, s, 2)[0].tobytes()
    out, w = _svm.svm_dca(x, y, alpha, w0, s, chains=2, want_w=True)
    assert w.tobytes() == _svm.dca_numpy(x, y, alpha, w0, s, 2)[1].tobytes()
    out = _svm.svm_dca(distarray.Absent((9, 3), f32), y, alpha, w0, s, chains=2, want_w=True)
    assert [type(t) for t in out] == [distarray.Absent] * 2
    assert [tuple(t.shape) for t in out] == [(9, 1), (2, 3)] and out[0].dtype == f32
    assert type(_svm.svm_dca(x, y, distarray.Absent((9, 1), f32), w0, s)) is distarray.Absent
    for bad in (x.astype(np.int32), x.astype(np.float16), x.astype(np.complex64)):
      both(TypeError, 'astype', xx=bad)
    both(TypeError, 'astype', yy=y.astype(np.int64))
    both(TypeError, 'astype', aa=alpha.astype(np.float64))
    both(TypeError, 'astype', ww=w0.astype(np.float64))
    both(ValueError, r'\(m, d\)', xx=x.reshape(-1))
    both(ValueError, r'\(m, d\)', xx=x.reshape(3, 3, 3))
    for bad in (y[:8], y.reshape(3, 3), y.reshape(1, 9)):
      both(ValueError, 'y of shape', yy=bad)
      both(ValueError, 'alpha of shape', aa=bad)
    for bad in (w0[:2], w0.reshape(1, 3), np.zeros((3, 2), f32)):
      both(ValueError, 'w0 of shape', ww=bad)
    both(ValueError, 'd = 0', xx=x[:, :0], ww=w0[:0])
    big = _hip.SP_SVM_MAX_D + 1
    both(ValueError, 'd = %d' % big, xx=np.zeros((2, big), f32), yy=y[:2], aa=alpha[:2], ww=np.zeros(big, f32))
    for chains in (0, -1):
      both(ValueError, 'chains', chains=chains)
    for bad in (0.0, -1.0, float('inf'), float('nan'), 1e-60, 1e60):     # (the last two: 0 and inf in float32)
      both(ValueError, 'scaled_lambda', ss=bad)
    x64 = [t.astype(np.float64) for t in (x, y, alpha, w0)]
    assert tile_checks.check_svm_dca([t.dtype for t in x64], [t.shape for t in x64], 1e-60, 3) == (np.dtype(np.float64), 9, 3, 1e-60, 3)
    ok = np.zeros((2, _hip.SP_SVM_MAX_D), f32)
    assert tile_checks.check_svm_dca([f32] * 4, [ok.shape, (2,), (2, 1), (ok.shape[1], 1)], 2, 5)[1:3] == (2, _hip.SP_SVM_MAX_D)
  finally:
    sp.shutdown()


def test_the_svm_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  header = os.path.join(ROOT, 'include', 'spartan_hip_svm.h')
  names = _declared_functions(header)
  assert names == sorted(_hip.EXPORTS_SVM) == ['sp_svm_dca']
  others = (set(_hip.EXPORTS) | set(_hip.EXPORTS_EXTRAS) | set(_hip.EXPORTS_EIG) | set(_hip.EXPORTS_KNN)
            | set(_hip.EXPORTS_GRAPH) | set(_hip.EXPORTS_ALS) | set(_hip.EXPORTS_FUZZY) | set(_hip.EXPORTS_LDA)
            | set(_hip.EXPORTS_SPECTRAL) | set(_hip.EXPORTS_NB) | set(_hip.EXPORTS_NBODY) | set(_hip.EXPORTS_CF))
  for h in (EXTRAS_HEADER,) + tuple(os.path.join(ROOT, 'include', 'spartan_hip_%s.h' % s)
                                    for s in ('eig', 'knn', 'graph', 'als', 'fuzzy', 'lda', 'spectral', 'nb', 'nbody', 'cf')):
    others |= set(_declared_functions(h))
  assert not set(names) & others
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  # the limit in three places: the header, the binding, and what the library itself takes
  text = open(header).read()
  assert int(re.search(r'#define SP_SVM_MAX_D (\d+)', text).group(1)) == _hip.SP_SVM_MAX_D == 4096
  x = _hip.extras()                                   # host code: a refusal and an empty call need no device
  f32, f64, top = _hip.SP_F32, _hip.SP_F64, _hip.SP_SVM_MAX_D
  one = ctypes.c_void_p(64)                           # (never read: nothing is launched)
  call = lambda dtype, m, d, ldx, s, chains, w0=one, rows=None: x.sp_svm_dca(  # noqa: E731
      dtype, rows, ldx, m, d, rows, rows, w0, s, chains, rows, None, None)
  assert call(f32, 0, top, top, 1.0, 1) == 0 == call(f64, 0, 1, 1, 0.5, 7)      # m = 0 without w_out: nothing to do
  assert call(f32, 0, top + 1, top + 1, 1.0, 1) != 0 and call(f32, 0, 0, 1, 1.0, 1) != 0
  assert call(_hip.SP_I32, 0, 4, 4, 1.0, 1) != 0 and call(f32, -1, 4, 4, 1.0, 1) != 0
  assert call(f32, 0, 4, 3, 1.0, 1) != 0 and call(f32, 0, 4, 4, 1.0, 0) != 0
  for s in (0.0, -1.0, float('inf'), float('nan'), 1e-60):
    assert call(f32, 0, 4, 4, s, 1) != 0
  assert call(f64, 0, 4, 4, 1e-60, 1) == 0
  assert call(f32, 0, 4, 4, 1.0, 1, w0=None) != 0 and call(f32, 3, 4, 4, 1.0, 1) != 0     # NULL pointers
