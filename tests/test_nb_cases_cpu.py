"""The NumPy restatement of the naive Bayes step (examples/_nb.py) against the longdouble oracle and the derived bound of
tests/nb_cases.py at every shape the device tests use, in both dtypes: the bound is not one only the kernel's luck
meets.  Also: the special values, `bad`, the refusals of the shared check, the composition against the reference's
recorded pieces, and that header, binding and library name the same two functions.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip
from spartan_amd.examples import _nb
from tests import nb_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = (np.float32, np.float64)
IDS = lambda s: '%dx%dx%d-%s' % s   # noqa: E731


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', nc.SHAPES, ids=IDS)
def test_the_numpy_body_meets_the_derived_bound(shape, dtype):
  m, d, label_size, kind = shape
  x, labels = nc.case(m, d, label_size, kind, np.dtype(dtype))
  want = nc.oracle_of_case(m, d, label_size, kind, np.dtype(dtype))
  s, df, bad = _nb.step_numpy(x, labels, label_size)
  share = nc.check_step(x, labels, label_size, s, df, bad, want=want, label='numpy %s %s' % (shape, np.dtype(dtype).name))
  assert share <= 1.0 and bad[0] == 0
  # its S is the row-order sum of its own z, bit for bit
  with np.errstate(all='ignore'):
    z = x / np.sqrt((x * x).sum(axis=1, dtype=x.dtype) / x.dtype.type(d))[:, None]
  assert s.tobytes() == nc.row_order_sum(z, labels, label_size).tobytes()
  if kind == 'equal':
    assert not np.any(s[:-1])
  used = np.zeros(label_size, bool)
  used[labels] = True
  assert not np.any(s[~used])                 # a label nobody has: zeros


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_special_values_in_the_numpy_body(dtype):
  dt = np.dtype(dtype)
  x, labels = (np.array(a) for a in nc.case(65, 7, 5, 'random', dt))
  base = _nb.step_numpy(x, labels, 5)
  zero = x.copy()
  zero[40] = 0
  s, df, bad = _nb.step_numpy(zero, labels, 5)
  nan_rows = np.isnan(s).all(axis=1)
  assert nan_rows.tolist() == [l == labels[40] for l in range(5)] and not np.isnan(s[~nan_rows]).any()
  assert s[~nan_rows].tobytes() == base[0][~nan_rows].tobytes() and bad[0] == 0
  nc.check_step(zero, labels, 5, s, df, bad, label='numpy zero row %s' % dt.name)
  neg = x.copy()
  neg[3, 2], neg[9, 4] = -2.0, np.nan
  s, df, bad = _nb.step_numpy(neg, labels, 5)
  assert df[2] == (x[:, 2] > 0).sum() - (x[3, 2] > 0) and df[4] == (x[:, 4] > 0).sum() - (x[9, 4] > 0)
  nc.check_step(neg, labels, 5, s, df, bad, label='numpy negative and NaN entries %s' % dt.name)
  for wrong in (-1, 5):
    lab = labels.copy()
    lab[[50, 12]] = wrong
    s, df, bad = _nb.step_numpy(x, lab, 5)
    assert bad.tolist() == [13] and df.tobytes() == base[1].tobytes()
    nc.check_step(x, lab, 5, s, df, bad, label='numpy label %d %s' % (wrong, dt.name))
    keep = np.ones(65, bool)
    keep[[50, 12]] = False
    assert s.tobytes() == _nb.step_numpy(x[keep], labels[keep], 5)[0].tobytes()
  s, df, bad = _nb.step_numpy(x[:0], labels[:0], 5)
  assert s.shape == (5, 7) and not s.any() and not df.any() and bad.tolist() == [0]
  s, df, bad = _nb.step_numpy(x[:, :0], labels, 5)
  assert s.shape == (5, 0) and df.shape == (0,) and bad.tolist() == [0]


def test_refusals_and_absent_tiles():
  from oracle.np_backend import NumpyBackend
  from spartan_amd.array import distarray
  sp.initialize(backend=NumpyBackend(), num_workers=1)
  try:
    x, labels = nc.case(9, 3, 2, 'random', np.dtype(np.float32))
    out = _nb.nb_step(x, labels.reshape(9, 1), 2)
    assert out[0].tobytes() == _nb.step_numpy(x, labels, 2)[0].tobytes()
    out = _nb.nb_step(distarray.Absent((9, 3), np.dtype(np.float32)), labels, 2)
    assert [type(t) for t in out] == [distarray.Absent] * 3
    assert [tuple(t.shape) for t in out] == [(2, 3), (3,), (1,)] and out[0].dtype == np.float32 and out[1].dtype == np.int64
    for bad in (x.astype(np.int32), x.astype(np.float16)):
      with pytest.raises(TypeError, match='astype'):
        _nb.nb_step(bad, labels, 2)
    for bad in (labels.astype(np.int32), labels.astype(np.float64)):
      with pytest.raises(TypeError, match='astype'):
        _nb.nb_step(x, bad, 2)
    for size in (0, 129, -3):
      with pytest.raises(ValueError, match='label_size'):
        _nb.nb_step(x, labels, size)
    with pytest.raises(ValueError, match=r'\(m, d\)'):
      _nb.nb_step(x.reshape(-1), labels, 2)
    for bad in (labels[:8], labels.reshape(3, 3), labels.reshape(1, 9)):
      with pytest.raises(ValueError, match='labels of shape'):
        _nb.nb_step(x, bad, 2)
  finally:
    sp.shutdown()


def test_the_numpy_body_composes_to_the_reference():
  """tests/golden/nb_w4.npz: the reference's mapper on its own normalised data, and its whole fit."""
  g = np.load(os.path.join(HERE, 'golden', 'nb_w4.npz'))
  data, labels, label_size, queries = nc.golden_input()
  assert g['data'].tobytes() == data.tobytes() and g['labels'].tobytes() == labels.tobytes()
  assert g['queries'].tobytes() == queries.tobytes()
  s, df, bad = _nb.step_numpy(data, labels, label_size)
  assert df.tobytes() == g['df'].tobytes() and bad[0] == 0
  n, d = data.shape
  idf = np.log(n * 1.0 / (df + 1)) + 1
  assert idf.tobytes() == g['idf'].tobytes()
  w = s * idf[None, :]
  scores = np.log((w + 1.0) / (w.sum(axis=1)[:, None] + 1.0 * d))
  want = nc.fit_oracle(data, labels, label_size, 1.0)
  ours = nc.fit_bound(want, data.shape, 1.0, np.float64, 'after')
  theirs = nc.fit_bound(want, data.shape, 1.0, np.float64, 'inside')
  for name, got, ref in (('W', w, g['W']), ('wl', w.sum(axis=1), g['wl']), ('scores', scores, g['scores'])):
    share = nc._ratio(np.abs(got - ref), ours[name] + theirs[name])
    ref_share = nc._ratio(np.abs(np.asarray(ref, nc.LD) - want[name]), theirs[name])
    print('%s: numpy body against the reference %.3g of the summed bounds; the reference against the oracle %.3g of its own'
          % (name, share, ref_share))
    assert share <= 1.0 and ref_share <= 1.0
  assert g['scores_per_label'].tobytes() == g['wl'].tobytes() or np.allclose(g['scores_per_label'], g['wl'], rtol=1e-12, atol=0)
  assert [int(np.argmax(scores.dot(q))) for q in queries] == g['predicted'].tolist()


def test_the_nb_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  header = os.path.join(ROOT, 'include', 'spartan_hip_nb.h')
  names = _declared_functions(header)
  assert names == sorted(_hip.EXPORTS_NB) == ['sp_nb_step', 'sp_nb_step_workspace_bytes']
  others = (set(_hip.EXPORTS) | set(_hip.EXPORTS_EXTRAS) | set(_hip.EXPORTS_EIG) | set(_hip.EXPORTS_KNN)
            | set(_hip.EXPORTS_GRAPH) | set(_hip.EXPORTS_ALS) | set(_hip.EXPORTS_FUZZY) | set(_hip.EXPORTS_LDA)
            | set(_hip.EXPORTS_SPECTRAL))
  for h in (EXTRAS_HEADER,) + tuple(os.path.join(ROOT, 'include', 'spartan_hip_%s.h' % s)
                                    for s in ('eig', 'knn', 'graph', 'als', 'fuzzy', 'lda', 'spectral')):
    others |= set(_declared_functions(h))
  assert not set(names) & others
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  x = _hip.extras()                                   # host code: sizes need no device
  f32, f64 = _hip.SP_F32, _hip.SP_F64
  size = x.sp_nb_step_workspace_bytes
  assert size(f32, 0, 6, 4, 0) == 256 == size(f32, 64, 6, 4, 7)                 # r alone: one block of rows is one range
  assert size(f64, 300, 70, 20, 1) == 2560                                      # 300 r of 8 bytes, rounded up to 256
  partial_s = -(-3 * 20 * 70 * 8 // 256) * 256                                  # three partial [label_size, d]
  partial_df = -(-3 * 70 * 8 // 256) * 256                                      # three partial df
  assert size(f64, 300, 70, 20, 3) == 2560 + partial_s + partial_df + 3 * 8     # ... and three first bad rows
  assert size(f64, 300, 70, 20, 7) == size(f64, 300, 70, 20, 5)                 # at most ceil(300 / 64) = 5 ranges
  assert size(f32, 960, 70, 20, 0) == size(f32, 960, 70, 20, 1)                 # under 16 blocks the library does not cut
  assert size(f32, 961, 70, 20, 0) == size(f32, 961, 70, 20, 2)                 # 16 blocks: two ranges of eight
  assert size(_hip.SP_I32, 300, 70, 20, 0) == 0 == size(f32, 300, 70, 0, 0) == size(f32, 300, 70, 129, 0)
  assert size(f32, -1, 4, 4, 0) == 0 == size(f32, 4, -1, 4, 0) == size(f32, 4, 4, 4, -1)
  assert _hip.SP_NB_MAX_LABELS == 128
