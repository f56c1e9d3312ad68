"""The SGD sequence on the CPU: tests/netflix_cases.restated against the reference's recorded _sgd_inner results byte
for byte (with the plain dot), the properties of sp_sgd_mf_plan's schedule on every case, sp_sgd_mf_host in plan order
and in tile order and examples/_netflix.sgd_numpy against restated byte for byte in both dtypes, the accuracy rule on
the golden input, the refusals of the shared check and of the plan function, and that header, binding and library name
the same functions and limits.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from spartan_amd import _hip, kernels, tile_checks
from spartan_amd.examples import _netflix
from tests import netflix_cases as nc

DTYPES = (np.float32, np.float64)
dtype_ids = dict(ids=lambda d: np.dtype(d).name)
CASE_NAMES = sorted(nc.cases(np.float32, _hip.SP_MF_WIDE))


def test_restated_with_the_plain_dot_is_the_reference_byte_for_byte():
  """f = 20, float32: everything but the order of the dot is pinned to the reference's compiled loop."""
  g = nc.golden()
  rows, cols, vals, u0, m0 = nc.golden_input()
  for k, v in (('rows', rows), ('cols', cols), ('vals', vals), ('U0', u0), ('M0', m0)):
    assert g[k].tobytes() == v.tobytes(), k
  assert int(g['whole_run']) == 1 and g['U_1'].dtype == np.float32
  strata = nc.golden_strata()
  assert len(strata) == nc.EPOCHS and all(sorted(b for st in ep for b in st) == [(i, j) for i in range(4) for j in range(4)]
                                          for ep in strata)
  got = nc.epochs(lambda *a: nc.restated(*a, dot='plain'), rows, cols, vals, u0, m0, strata)
  for t in range(nc.EPOCHS):
    assert got[t][0].tobytes() == g['U_%d' % (t + 1)].tobytes() and got[t][1].tobytes() == g['M_%d' % (t + 1)].tobytes()
  assert np.abs(g['U_2'] - u0).max() > 100 * nc.FACTOR * nc.e_ref()          # (a run that does nothing cannot pass)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_accuracy_against_the_reference(dtype):
  rows, cols, vals, u0, m0 = nc.golden_input()
  got = nc.epochs(nc.restated, rows, cols, vals, u0, m0, nc.golden_strata(), dtype=dtype)
  nc.check_accuracy(got, dtype, 'restated')


@pytest.mark.parametrize('name', CASE_NAMES)
def test_plan_properties(name):
  shape, (indptr, indices, _) = nc.cases(np.float32, _hip.SP_MF_WIDE)[name]
  nnz = len(indices)
  plan = kernels.sgd_mf_plan(shape[0], shape[1], indptr, indices)
  p = kernels.sgd_mf_plan_parts(plan)
  assert (p['m'], p['n'], p['nnz'], p['wide']) == (shape[0], shape[1], nnz, _hip.SP_MF_WIDE)
  assert len(plan) == int(plan[:64].view(np.int64)[6]) and len(plan) <= _hip.extras().sp_sgd_mf_plan_bytes(shape[0], shape[1], nnz)
  rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
  entry, off = p['entry'], p['level_off']
  assert sorted(entry.tolist()) == list(range(nnz))                                  # each entry once
  assert p['row'].tolist() == rows[entry].tolist() and p['col'].tolist() == indices[entry].tolist()
  assert off[0] == 0 and off[-1] == nnz and (np.diff(off) > 0).all()                 # levels non-decreasing, none empty
  level = np.empty(nnz, np.int64)
  for v in range(p['levels']):
    mine = entry[off[v]:off[v + 1]]
    level[mine] = v
    assert (np.diff(mine) > 0).all()                                                 # ascending inside a level
    assert len(set(rows[mine])) == len(mine) == len(set(indices[mine]))              # no shared row, no shared column
  # each entry after its predecessors in its row and in its column -- and directly after the later of them
  rowlast, collast = {}, {}
  for e in range(nnz):
    i, j = rows[e], indices[e]
    before = [level[x] for x in (rowlast.get(i), collast.get(j)) if x is not None]
    assert level[e] == (max(before) + 1 if before else 0)
    rowlast[i] = collast[j] = e
  # the segments tile the levels; a wide segment is one level of at least SP_MF_WIDE, narrow runs are maximal
  widths = np.diff(off)
  at, last = 0, None
  for kind, lv0, lv1, zero in p['segments'].tolist():
    assert lv0 == at and lv1 > lv0 and zero == 0 and kind in (0, 1)
    if kind == 1:
      assert lv1 == lv0 + 1 and widths[lv0] >= _hip.SP_MF_WIDE
    else:
      assert (widths[lv0:lv1] < _hip.SP_MF_WIDE).all() and last != 0
    at, last = lv1, kind
  assert at == p['levels']


def test_the_wide_cases_have_both_kinds_of_segment():
  w = _hip.SP_MF_WIDE
  kinds = {}
  for name, (shape, (indptr, indices, _)) in nc.cases(np.float32, w).items():
    p = kernels.sgd_mf_plan_parts(kernels.sgd_mf_plan(shape[0], shape[1], indptr, indices))
    kinds[name] = p['segments'][:, 0].tolist()
  assert kinds['pairs'] == [1] and kinds['pairs and their successors'] == [1, 1, 0]
  assert kinds['narrow wide narrow'] == [0, 1, 0] and set(kinds['13 x 1250']) == {0} == set(kinds['pairs shifted by one column'])
  assert kinds['empty'] == []


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('name', CASE_NAMES)
def test_plan_order_is_tile_order_is_restated_byte_for_byte(name, dtype):
  shape, (indptr, indices, vals) = nc.cases(dtype, _hip.SP_MF_WIDE)[name]
  nnz = len(indices)
  order = kernels.sgd_mf_plan_parts(kernels.sgd_mf_plan(shape[0], shape[1], indptr, indices))['entry']
  for f in ((7, 20, 65) if name in ('13 x 1250', 'special values') else (20,)):
    u0, m0 = nc.factors(shape[0], shape[1], f, dtype, ld_extra=3)
    want_u, want_m, want_e = nc.restated(indptr, indices, vals, u0, m0)
    for how in ('tile order', 'plan order', 'numpy'):
      u, m = nc.factors(shape[0], shape[1], f, dtype, ld_extra=3)
      err = np.zeros(nnz, dtype)
      if how == 'numpy':
        _netflix.sgd_numpy(indptr, indices, vals, u, m, nc.LR, err)
      else:
        kernels.sgd_mf_host(shape, indptr, indices, vals, u, m, None, err, order if how == 'plan order' else None)
      assert nc.same(u, want_u) and nc.same(m, want_m) and nc.same(err, want_e), (name, f, how)
      assert (u.base[:, f:] == 7).all() and (m.base[:, f:] == 7).all()              # nothing outside the f columns
    if nnz and name != 'special values':
      assert u.tobytes() == want_u.tobytes() and not np.array_equal(u, u0)
  if name == 'special values':
    marks = nc.special_tile(dtype)[2]
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    for k in ('nan', 'inf'):                         # both of the rating's rows are poisoned ...
      assert not np.isfinite(want_u[rows[marks[k]]]).any() and not np.isfinite(want_m[indices[marks[k]]]).any()
    assert rows[marks['zero']] >= 6                  # ... entries that touch neither are unaffected; 0 is a rating
    assert np.isfinite(want_u[6:]).all() and np.isfinite(want_m[40:]).all() and want_e[marks['zero']] > 0.1
    assert want_u[6:].tobytes() != u0[6:].tobytes()


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_lane_dot_is_the_stated_dot(dtype):
  rng = np.random.RandomState(3)
  for f in nc.RANKS:
    p, q = rng.randn(f).astype(dtype), rng.randn(f).astype(dtype)
    assert _netflix.lane_dot(p, q).tobytes() == nc.stated_dot(p, q).tobytes()
    assert _netflix.lanes_of(f) == nc.lanes_of(f)


def test_refusals_of_the_check():
  f32, f64 = np.dtype(np.float32), np.dtype(np.float64)
  ok = tile_checks.check_sgd_mf([f32] * 3, (5, 9), (5, 20), (9, 20))
  assert ok == (f32, 5, 9, 20, float(np.float32(1e-5)))
  assert tile_checks.check_sgd_mf([f64] * 3, (5, 9), (5, 512), (9, 512), 0.5)[3:] == (512, 0.5)
  for bad in (np.int32, np.float16, np.complex64):
    with pytest.raises(TypeError, match='astype'):
      tile_checks.check_sgd_mf([f32, bad, f32], (5, 9), (5, 20), (9, 20))
  with pytest.raises(TypeError, match='astype'):
    tile_checks.check_sgd_mf([f32, f32, f64], (5, 9), (5, 20), (9, 20))
  with pytest.raises(ValueError, match=r'\(m, n\)'):
    tile_checks.check_sgd_mf([f32] * 3, (45,), (5, 20), (9, 20))
  for u in ((4, 20), (5,), (5, 20, 1)):
    with pytest.raises(ValueError, match='U of shape'):
      tile_checks.check_sgd_mf([f32] * 3, (5, 9), u, (9, 20))
  for m in ((9, 19), (8, 20), (9,)):
    with pytest.raises(ValueError, match='M of shape'):
      tile_checks.check_sgd_mf([f32] * 3, (5, 9), (5, 20), m)
  for f in (0, _hip.SP_MF_MAX_F + 1):
    with pytest.raises(ValueError, match='rank f = %d' % f):
      tile_checks.check_sgd_mf([f32] * 3, (5, 9), (5, f), (9, f))
  for lr in (float('nan'), float('inf'), 1e60):
    with pytest.raises(ValueError, match='lr'):
      tile_checks.check_sgd_mf([f32] * 3, (5, 9), (5, 20), (9, 20), lr)
  assert tile_checks.check_sgd_mf([f64] * 3, (5, 9), (5, 20), (9, 20), 1e60)[4] == 1e60


def test_refusals_of_the_plan_and_the_host_loop():
  x = _hip.extras()
  indptr = np.array([0, 2, 3], np.int64)
  indices = np.array([0, 4, 2], np.int32)
  need = x.sp_sgd_mf_plan_bytes(2, 5, 3)
  buf = np.zeros(need // 8 + 1, np.int64)
  plan = lambda m, n, nnz, ip, ix, size=need: x.sp_sgd_mf_plan(m, n, nnz, ip.ctypes.data, ix.ctypes.data, buf.ctypes.data, size)  # noqa: E731
  assert plan(2, 5, 3, indptr, indices) == 0
  assert x.sp_sgd_mf_plan_bytes(2, 5, 2 ** 31) == 0 and x.sp_sgd_mf_plan_bytes(-1, 5, 3) == 0
  assert plan(2, 5, 2 ** 31, indptr, indices) != 0                                     # nnz >= 2^31
  assert plan(2, 5, 3, np.array([0, 3, 2], np.int64), indices) != 0                    # indptr not monotone
  assert plan(2, 5, 3, np.array([0, 2, 2], np.int64), indices) != 0                    # indptr[m] != nnz
  assert plan(2, 5, 3, np.array([1, 2, 3], np.int64), indices) != 0                    # indptr[0] != 0
  assert plan(2, 4, 3, indptr, indices) != 0                                           # index 4 outside 0 .. 3
  assert plan(2, 5, 3, indptr, np.array([0, -1, 2], np.int32)) != 0
  assert plan(2, 5, 3, indptr, indices, need - 1) != 0 and plan(-1, 5, 3, indptr, indices) != 0
  with pytest.raises(_hip.HipError, match='outside'):
    kernels.sgd_mf_plan(2, 4, indptr, indices)
  # the host loop: the shared check first, then the library
  vals = np.ones(3, np.float32)
  u, m = nc.factors(2, 5, 4, np.float32)
  with pytest.raises(ValueError, match='lr'):
    kernels.sgd_mf_host((2, 5), indptr, indices, vals, u, m, float('nan'))
  with pytest.raises(TypeError, match='astype'):
    kernels.sgd_mf_host((2, 5), indptr, indices, vals.astype(np.float64), u, m)
  with pytest.raises(_hip.HipError, match='no entry'):
    kernels.sgd_mf_host((2, 5), indptr, indices, vals, u, m, order=np.array([0, 1, 3], np.int32))
  with pytest.raises(_hip.HipError, match='monotone'):
    kernels.sgd_mf_host((2, 5), np.array([0, 4, 3], np.int64), indices, vals, u, m)


def test_the_mf_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  header = os.path.join(ROOT, 'include', 'spartan_hip_mf.h')
  names = _declared_functions(header)
  assert names == sorted(_hip.EXPORTS_MF) == ['sp_sgd_mf', 'sp_sgd_mf_host', 'sp_sgd_mf_plan', 'sp_sgd_mf_plan_bytes']
  others = (set(_hip.EXPORTS) | set(_hip.EXPORTS_EXTRAS) | set(_hip.EXPORTS_EIG) | set(_hip.EXPORTS_KNN)
            | set(_hip.EXPORTS_GRAPH) | set(_hip.EXPORTS_ALS) | set(_hip.EXPORTS_FUZZY) | set(_hip.EXPORTS_LDA)
            | set(_hip.EXPORTS_SPECTRAL) | set(_hip.EXPORTS_NB) | set(_hip.EXPORTS_NBODY) | set(_hip.EXPORTS_CF)
            | set(_hip.EXPORTS_SVM))
  for h in (EXTRAS_HEADER,) + tuple(os.path.join(ROOT, 'include', 'spartan_hip_%s.h' % s)
                                    for s in ('eig', 'knn', 'graph', 'als', 'fuzzy', 'lda', 'spectral', 'nb', 'nbody', 'cf', 'svm')):
    others |= set(_declared_functions(h))
  assert not set(names) & others
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  text = open(header).read()
  assert int(re.search(r'#define SP_MF_MAX_F (\d+)', text).group(1)) == _hip.SP_MF_MAX_F == 512
  assert int(re.search(r'#define SP_MF_WIDE (\d+)', text).group(1)) == _hip.SP_MF_WIDE
  # what the library itself takes, without a device: refusals come before any launch, and an empty tile launches nothing
  x = _hip.extras()
  f32, top = _hip.SP_F32, _hip.SP_MF_MAX_F
  one = ctypes.c_void_p(64)                          # (never read: nothing is launched)
  n = ctypes.c_int64(-1)
  call = lambda dtype, m, nn, f, nnz, ldu, ldm, lr, p=one: x.sp_sgd_mf(dtype, m, nn, f, nnz, p, p, p, p, ldu, p, ldm, lr, None,  # noqa: E731
                                                                    ctypes.byref(n), None)
  assert call(f32, 3, 4, top, 0, top, top, 1e-5) == 0 and n.value == 0
  assert call(_hip.SP_F64, 0, 0, 1, 0, 1, 1, 0.0) == 0
  assert call(_hip.SP_I32, 3, 4, 5, 0, 5, 5, 1e-5) != 0
  assert call(f32, 3, 4, top + 1, 0, top + 1, top + 1, 1e-5) != 0 and call(f32, 3, 4, 0, 0, 1, 1, 1e-5) != 0
  assert call(f32, 3, 4, 5, 0, 4, 5, 1e-5) != 0 and call(f32, 3, 4, 5, 0, 5, 4, 1e-5) != 0
  assert call(f32, -1, 4, 5, 0, 5, 5, 1e-5) != 0 and call(f32, 3, 4, 5, -1, 5, 5, 1e-5) != 0
  for lr in (float('nan'), float('inf'), 1e60):
    assert call(f32, 3, 4, 5, 0, 5, 5, lr) != 0
  assert call(f32, 3, 4, 5, 2, 5, 5, 1e-5, p=None) != 0                                # NULL operands where nnz > 0
  junk = np.zeros(64, np.int64)                                                        # a plan without the magic number
  assert x.sp_sgd_mf(f32, 3, 4, 5, 2, one, one, junk.ctypes.data, one, 5, one, 5, 1e-5, None, None, None) != 0


def test_the_numpy_body_and_absent_tiles():
  """_netflix.sgd_mf on a backend without the method: the NumPy body, in place; Absent operands compute nothing."""
  import scipy.sparse as sps

  import spartan_amd as sp
  from oracle.np_backend import NumpyBackend
  from spartan_amd.array import distarray
  f32 = np.dtype(np.float32)
  shape, (indptr, indices, vals) = nc.cases(f32, _hip.SP_MF_WIDE)['dense 8 x 8']
  u0, m0 = nc.factors(8, 8, 5, f32)
  want_u, want_m, want_e = nc.restated(indptr, indices, vals, u0, m0)
  sp.initialize(backend=NumpyBackend(), num_workers=1)
  try:
    v = sps.csr_matrix((vals, indices, indptr), shape=shape)
    u, m = np.array(u0), np.array(m0)
    assert _netflix.sgd_mf(v, u, m) is None
    assert u.tobytes() == want_u.tobytes() and m.tobytes() == want_m.tobytes()
    u, m = np.array(u0), np.array(m0)
    total = _netflix.sgd_mf(v.tocoo(), u, m, want_error=True)
    assert total.shape == (1, 1) and total.dtype == f32 and abs(float(total[0, 0]) - float(want_e.sum(dtype=np.float64))) < 1e-3
    assert u.tobytes() == want_u.tobytes()
    u, m = np.array(u0), np.array(m0)
    assert _netflix.sgd_mf(distarray.Absent(shape, f32), u, m) is None
    out = _netflix.sgd_mf(v, distarray.Absent((8, 5), f32), m, want_error=True)
    assert type(out) is distarray.Absent and tuple(out.shape) == (1, 1) and out.dtype == f32
    assert u.tobytes() == u0.tobytes() and m.tobytes() == m0.tobytes()
    with pytest.raises(ValueError, match='U of shape'):
      _netflix.sgd_mf(distarray.Absent(shape, f32), u[:7], m)
    with pytest.raises(TypeError, match='astype'):
      _netflix.sgd_mf(v, u.astype(np.float64), m)
    with pytest.raises(ValueError, match='lr'):
      _netflix.sgd_mf(v, u, m, lr=float('inf'))
  finally:
    sp.shutdown()
