"""The NumPy bodies of canopy clustering (examples/_canopy.canopy_numpy, pdf_label_numpy) against the reference's own
mappers recorded in tests/golden/canopy_w4.npz, byte for byte in float64; chain independence; the rounding tie that
separates the label from an arg-min of the distance; the refusals of the two shared checks; placeholders; and that
header, binding and library name the same functions.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, tile_checks
from spartan_amd.examples import _canopy, canopy_clustering as cc
from tests import canopy_cases as case

SETTINGS = range(len(case.SETTINGS))


def _filtered(x, t1, t2, chains=1):
  centers, counts, rows = _canopy.canopy_numpy(x, t1, t2, chains)
  return centers[counts > case.CF]


@pytest.mark.parametrize('s', SETTINGS)
def test_the_numpy_bodies_are_the_reference_byte_for_byte(s):
  g = case.golden()
  x, t1, t2 = case.golden_input(s)
  before = x.copy()
  blocks = []
  for b, (lo, hi) in enumerate(case.bands()):
    got = _filtered(x[lo:hi], t1, t2)
    assert case.same(got, g['band_%d_%d' % (s, b)]), (s, b)
    blocks.append(got)
  # find_centers: the same loop over the bands' results in ascending order
  centers = _filtered(np.concatenate(blocks), t1, t2)
  assert case.same(centers, g['centers_%d' % s])
  labels = _canopy.pdf_label_numpy(x, centers)
  assert case.same(labels, g['labels_%d' % s]) and labels.dtype == np.int32
  assert x.tobytes() == before.tobytes()                  # no operand is written
  assert len(centers) >= 4 and len(set(labels.tolist())) >= 3
  if int(g['whole_run_%d' % s]):                          # (the reference's own driver, where it evaluated)
    if g['run_order_%d' % s].tolist() == list(range(case.WORKERS)):
      assert case.same(labels, g['run_labels_%d' % s])


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('s', SETTINGS)
def test_chains_are_calls_on_the_bands(s, dtype):
  x, t1, t2 = case.golden_input(s)
  x = x.astype(dtype)
  whole = _canopy.canopy_numpy(x, t1, t2, case.WORKERS)
  parts = [_canopy.canopy_numpy(x[lo:hi], t1, t2) for lo, hi in case.chain_rows(len(x), case.WORKERS)]
  assert case.chain_rows(len(x), case.WORKERS) == case.bands()
  assert case.same(whole[0], np.concatenate([p[0] for p in parts])) and whole[0].dtype == np.dtype(dtype)
  assert case.same(whole[1], np.concatenate([p[1] for p in parts])) and whole[1].dtype == np.int64
  offsets = [lo for lo, _ in case.bands()]
  assert case.same(whole[2], np.concatenate([p[2] + lo for p, lo in zip(parts, offsets)]))
  # a creating row is a row of x, a count is at least 1, and every count is the rows within t1 of the creating row
  # from it onwards in its band
  assert (whole[1] >= 1).all() and case.chain_rows(7, 10)[:3] == [(0, 0), (0, 1), (1, 2)]
  # more chains than rows: chains without rows make nothing
  few = _canopy.canopy_numpy(x[:3], t1, t2, 7)
  assert few[2].tolist() == [0, 1, 2] and few[1].tolist() == [1, 1, 1] and case.same(few[0], x[:3])
  empty = _canopy.canopy_numpy(x[:0], t1, t2, 2)
  assert [a.shape for a in empty] == [(0, x.shape[1]), (0,), (0,)]


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_the_loop_by_hand(dtype):
  """Integer coordinates: every distance is exact.  Strict <: a row at squared distance exactly t2 is not bound, one at
  exactly t1 is not observed; a duplicate of a creating row is observed; a row with a NaN is a canopy of its own."""
  x = np.array([[0, 0], [2, 0], [0, 0], [1, 0], [3, 0], [np.nan, 0], [0, 1]], dtype)
  centers, counts, rows = _canopy.canopy_numpy(x, 4, 4)
  # row 1: d2 = 4 to row 0, not < 4: a canopy.  row 2: the duplicate, observed by 0 (d2 = 0), not by 1 (d2 = 4).
  # row 3: within 4 of both.  row 4: d2 = 9 and 1.  row 5: NaN.  row 6: d2 = 1 to row 0, 5 to row 1.
  assert rows.tolist() == [0, 1, 5] and counts.tolist() == [4, 3, 1]
  want = np.array([[(0 + 0 + 1 + 0) / 4, 1 / 4], [(2 + 1 + 3) / 3, 0], [np.nan, 0]], dtype)
  assert case.same(centers, want)
  # t1 < t2: bound without being observed; t1 > t2: observed and a canopy as well
  centers, counts, rows = _canopy.canopy_numpy(x[:5], 1, 5)
  assert rows.tolist() == [0, 4] and counts.tolist() == [2, 1]
  centers, counts, rows = _canopy.canopy_numpy(x[:5], 5, 1)
  assert rows.tolist() == [0, 1, 3, 4] and counts.tolist() == [4, 4, 2, 1]
  assert case.same(centers, np.array([[3 / 4, 0], [6 / 4, 0], [2, 0], [3, 0]], dtype))


@pytest.mark.parametrize('dtype', (np.float32, np.float64), ids=lambda d: np.dtype(d).name)
def test_the_label_is_not_an_arg_min_of_the_distance(dtype):
  """1 + 1e-20 rounds to 1 in both dtypes: the farther centre, listed first, ties with the nearer one and wins."""
  x = np.array([[0.0, 0.0], [5.0, 5.0]], dtype)
  centers = np.array([[1e-10, 0.0], [0.0, 0.0], [5.0, 5.0]], dtype)
  d2 = np.square(x[0] - centers).sum(axis=1)
  assert d2[0] > d2[1] == 0 and int(np.argmin(d2)) == 1
  labels = _canopy.pdf_label_numpy(x, centers)
  assert labels.tolist() == [0, 2] and labels.dtype == np.int32
  # no centre: -1; a NaN pdf never wins; all NaN: -1
  assert _canopy.pdf_label_numpy(x, centers[:0]).tolist() == [-1, -1]
  nan_first = np.array([[np.nan, 0.0], [5.0, 5.0]], dtype)
  assert _canopy.pdf_label_numpy(x, nan_first).tolist() == [1, 1]
  assert _canopy.pdf_label_numpy(np.array([[np.nan, 0.0], [0.0, 0.0]], dtype), centers).tolist() == [-1, 0]
  # an infinite distance has pdf 0, which beats the -1 the search starts from
  assert _canopy.pdf_label_numpy(x, np.array([[np.inf, 0.0]], dtype)).tolist() == [0, 0]


def test_refusals_and_absent_tiles():
  from oracle.np_backend import NumpyBackend
  from spartan_amd.array import distarray
  f32 = np.dtype(np.float32)
  x, t1, t2 = case.golden_input(0)
  x = x[:9].astype(f32)
  centers = x[:2].copy()

  def canopy_both(exc, match, xx=x, a1=t1, a2=t2, chains=1, cap=None):
    """The check and the dispatcher (here: the NumPy body) refuse alike."""
    with pytest.raises(exc, match=match):
      tile_checks.check_canopy(xx.dtype, xx.shape, a1, a2, chains, cap)
    with pytest.raises(exc, match=match):
      _canopy.canopy(xx, a1, a2, chains=chains, cap=cap)

  def label_both(exc, match, xx=x, cc_=centers):
    with pytest.raises(exc, match=match):
      tile_checks.check_pdf_label([xx.dtype, cc_.dtype], [xx.shape, cc_.shape])
    with pytest.raises(exc, match=match):
      _canopy.pdf_label(xx, cc_)

  sp.initialize(backend=NumpyBackend(), num_workers=1)
  try:
    got = _canopy.canopy(x, t1, t2, chains=2)
    assert all(case.same(a, b) for a, b in zip(got, _canopy.canopy_numpy(x, t1, t2, 2)))
    assert case.same(_canopy.pdf_label(x, centers), _canopy.pdf_label_numpy(x, centers))
    out = _canopy.canopy(distarray.Absent((9, 3), f32), t1, t2, chains=2)
    assert [type(t) for t in out] == [distarray.Absent] * 3
    assert [tuple(t.shape) for t in out] == [(0, 3), (0,), (0,)] and out[0].dtype == f32 and out[1].dtype == np.int64
    for operands in ((distarray.Absent((9, 3), f32), centers), (x, distarray.Absent((2, 3), f32))):
      lab = _canopy.pdf_label(*operands)
      assert type(lab) is distarray.Absent and lab.shape == (9,) and lab.dtype == np.int32
    with pytest.raises(TypeError, match='astype'):
      _canopy.canopy(distarray.Absent((9, 3), np.int32), t1, t2)

    for bad in (x.astype(np.int32), x.astype(np.float16), x.astype(np.complex64)):
      canopy_both(TypeError, 'astype', xx=bad)
      label_both(TypeError, 'astype', xx=bad)
      label_both(TypeError, 'astype', cc_=bad[:2])
    label_both(TypeError, 'astype', cc_=centers.astype(np.float64))      # mixed
    canopy_both(ValueError, r'\(n, d\)', xx=x.reshape(-1))
    canopy_both(ValueError, r'\(n, d\)', xx=x.reshape(3, 3, 3))
    label_both(ValueError, r'\(n, d\)', xx=x.reshape(-1))
    label_both(ValueError, r'\(k, d\)', cc_=centers.reshape(-1))
    label_both(ValueError, 'features', cc_=centers[:, :2])
    canopy_both(ValueError, 'd = 0', xx=x[:, :0])
    label_both(ValueError, 'd = 0', xx=x[:, :0], cc_=centers[:, :0])
    for bad in (0, -1):
      canopy_both(ValueError, 'chains', chains=bad)
      canopy_both(ValueError, 'cap', cap=bad)
    for bad in (float('inf'), float('nan'), -float('inf'), 1e60):        # (the last: inf in float32)
      canopy_both(ValueError, 't1', a1=bad)
      canopy_both(ValueError, 't2', a2=bad)
    for bad in (1.5, 1.0, '1', None, True):
      with pytest.raises(ValueError, match='cf'):
        cc.find_centers([x], t1, t2, bad)
      with pytest.raises(ValueError, match='cf'):
        cc.canopy_cluster(x, t1, t2, cf=bad)
    # what the checks return: the default cap is min(the longest chain, 1024), at least 1
    assert tile_checks.check_canopy(np.float64, (9, 3), 1e60, 2, 2) == (np.dtype(np.float64), 9, 3, 1e60, 2.0, 2, 5, None)
    assert tile_checks.check_canopy(f32, (5000, 3), 1, 2, 3, cf=np.int64(4))[5:] == (3, 1024, 4)
    assert tile_checks.check_canopy(f32, (0, 3), 1, 2, 3, cap=7)[5:7] == (3, 7)
    assert tile_checks.check_canopy(f32, (0, 3), 1, 2)[6] == 1
    assert tile_checks.check_pdf_label([f32, f32], [(9, 3), (0, 3)]) == (f32, 9, 0, 3)
  finally:
    sp.shutdown()


def test_the_canopy_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  header = os.path.join(ROOT, 'include', 'spartan_hip_canopy.h')
  names = _declared_functions(header)
  assert names == sorted(_hip.EXPORTS_CANOPY) == ['sp_canopy', 'sp_canopy_workspace_bytes', 'sp_pdf_label']
  others = (set(_hip.EXPORTS) | set(_hip.EXPORTS_EXTRAS) | set(_hip.EXPORTS_EIG) | set(_hip.EXPORTS_KNN)
            | set(_hip.EXPORTS_GRAPH) | set(_hip.EXPORTS_ALS) | set(_hip.EXPORTS_FUZZY) | set(_hip.EXPORTS_LDA)
            | set(_hip.EXPORTS_SPECTRAL) | set(_hip.EXPORTS_NB) | set(_hip.EXPORTS_NBODY) | set(_hip.EXPORTS_CF)
            | set(_hip.EXPORTS_SVM) | set(_hip.EXPORTS_MF) | set(_hip.EXPORTS_LMM))
  for h in (EXTRAS_HEADER,) + tuple(os.path.join(ROOT, 'include', 'spartan_hip_%s.h' % s)
                                    for s in ('eig', 'knn', 'graph', 'als', 'fuzzy', 'lda', 'spectral', 'nb', 'nbody', 'cf',
                                              'svm', 'mf', 'lmm')):
    others |= set(_declared_functions(h))
  assert not set(names) & others
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  # the workspace query is host code: the creating rows of every slot, 256-byte aligned; 0 for what sp_canopy refuses
  x = _hip.extras()
  f32, f64 = _hip.SP_F32, _hip.SP_F64
  assert x.sp_canopy_workspace_bytes(f32, 100, 3, 2, 50) == 1280 and x.sp_canopy_workspace_bytes(f64, 100, 3, 2, 50) == 2560
  assert x.sp_canopy_workspace_bytes(f32, 0, 1, 1, 1) == 256
  for bad in ((_hip.SP_I32, 100, 3, 2, 50), (f32, -1, 3, 2, 50), (f32, 100, 0, 2, 50), (f32, 100, 3, 0, 50),
              (f32, 100, 3, 2, 0)):
    assert x.sp_canopy_workspace_bytes(*bad) == 0


def test_the_mixin():
  from spartan_amd.backend_hip import HipBackend
  from spartan_amd.backend_hip_canopy import CanopyTileBodies
  assert issubclass(HipBackend, CanopyTileBodies)
  assert [m for m in vars(CanopyTileBodies) if not m.startswith('_')] == ['canopy', 'pdf_label']
