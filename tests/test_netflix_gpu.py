"""sp_sgd_mf (csrc/sgd_mf.hip) through HipBackend.sgd_mf and kernels.sgd_mf against the sequence of
tests/netflix_cases.restated -- one entry at a time, no schedule -- byte for byte, U, M and |d| alike, in both dtypes.

Shapes, the smallest at which the kernel can go wrong (include/spartan_hip_mf.h): the ranks 1, 7, 16, 17, 20, 64, 65,
500 and 512 lie on both sides of every lanes-per-rating boundary; the structures are those of netflix_cases.cases -- an
empty tile, one row (every level one entry), one column, a dense 8 x 8 block (anti-diagonals), 13 x 1250 with about 975
entries (narrow levels only), and the wide cases built from SP_MF_WIDE: one wide level, two wide levels of which the
second depends on the first, then a narrow tail, and narrow -> wide -> narrow.  Every U and M is a row view of an array
three columns wider."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, kernels, tile_checks
from spartan_amd import sparse as sparse_mod
from tests import netflix_cases as nc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
dtype_ids = dict(ids=lambda d: np.dtype(d).name)
CASE_NAMES = sorted(nc.cases(np.float32, _hip.SP_MF_WIDE))
_restated = {}


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _tile(be, shape, indptr, indices, vals):
  return sparse_mod.CsrTile(shape, vals.dtype, be.from_numpy(indptr), be.from_numpy(indices), be.from_numpy(vals))


def _want(name, f, dtype):
  """restated on a case, computed once and never written."""
  key = (name, f, np.dtype(dtype).name)
  if key not in _restated:
    shape, (indptr, indices, vals) = nc.cases(dtype, _hip.SP_MF_WIDE)[name]
    u0, m0 = nc.factors(shape[0], shape[1], f, dtype, ld_extra=3)
    _restated[key] = nc.restated(indptr, indices, vals, u0, m0)
  return _restated[key]


def _run(be, name, f, dtype, want_error=True):
  """(U', M', |d|, the plan's parts) of one pass on the device, U and M being row views of wider arrays."""
  shape, (indptr, indices, vals) = nc.cases(dtype, _hip.SP_MF_WIDE)[name]
  u0, m0 = nc.factors(shape[0], shape[1], f, dtype, ld_extra=3)
  ud, md = be.from_numpy(u0.base), be.from_numpy(m0.base)
  t = _tile(be, shape, indptr, indices, vals)
  before = be.launches
  err = be.sgd_mf(t, ud[:, :f], md[:, :f], want_error=want_error)
  assert be.launches - before == (1 if len(indices) else 0)
  got_u, got_m = ud.numpy(), md.numpy()
  assert (got_u[:, f:] == 7).all() and (got_m[:, f:] == 7).all()                   # nothing outside the f columns
  parts = kernels.sgd_mf_plan_parts(sparse_mod.sgd_mf_plan(t)[0]) if len(indices) else None
  return got_u[:, :f], got_m[:, :f], (err.numpy() if want_error else None), parts, (t, ud, md)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('f', nc.RANKS)
def test_ranks(be, f, dtype):
  """Every lanes-per-rating path on a narrow-only tile and on the narrow -> wide -> narrow one."""
  for name in ('13 x 1250', 'narrow wide narrow') if f <= 65 else ('narrow wide narrow',):
    got_u, got_m, got_e, _, _ = _run(be, name, f, dtype)
    want_u, want_m, want_e = _want(name, f, dtype)
    assert got_u.tobytes() == want_u.tobytes() and got_m.tobytes() == want_m.tobytes(), (name, f)
    assert got_e.tobytes() == want_e.tobytes(), (name, f)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('name', CASE_NAMES)
def test_structures(be, name, dtype):
  f = 20
  got_u, got_m, got_e, parts, _ = _run(be, name, f, dtype)
  want_u, want_m, want_e = _want(name, f, dtype)
  assert nc.same(got_u, want_u) and nc.same(got_m, want_m) and nc.same(got_e, want_e), name
  if name != 'special values':
    assert got_u.tobytes() == want_u.tobytes() and got_m.tobytes() == want_m.tobytes() and got_e.tobytes() == want_e.tobytes()
  if parts is not None:
    kinds = parts['segments'][:, 0].tolist()
    want_kinds = {'pairs': [1], 'pairs and their successors': [1, 1, 0], 'narrow wide narrow': [0, 1, 0]}.get(name)
    assert kinds == want_kinds if want_kinds else set(kinds) == {0}
    if name == 'one row':
      assert parts['levels'] == parts['nnz']                                       # width 1, depth = nnz
    if name == 'dense 8 x 8':
      assert np.diff(parts['level_off']).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 7, 6, 5, 4, 3, 2, 1]
    if name == '13 x 1250':
      assert parts['levels'] > 90 and np.diff(parts['level_off']).max() <= 13
  # without the error terms: the same factors
  u2, m2, _, _, _ = _run(be, name, f, dtype, want_error=False)
  assert nc.same(u2, want_u) and nc.same(m2, want_m)


def test_both_kinds_of_segment_and_both_transitions_occur(be):
  """The wide cases are built from SP_MF_WIDE: read off the plans the device tests above ran with."""
  seen, moves = set(), set()
  for name in CASE_NAMES:
    shape, (indptr, indices, _) = nc.cases(np.float32, _hip.SP_MF_WIDE)[name]
    if len(indices):
      kinds = kernels.sgd_mf_plan_parts(kernels.sgd_mf_plan(shape[0], shape[1], indptr, indices))['segments'][:, 0].tolist()
      seen |= set(kinds)
      moves |= set(zip(kinds, kinds[1:]))
  assert seen == {0, 1} and {(0, 1), (1, 0), (1, 1)} <= moves


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_special_values(be, dtype):
  got_u, got_m, got_e, _, _ = _run(be, 'special values', 20, dtype)
  want_u, want_m, want_e = _want('special values', 20, dtype)
  assert nc.same(got_u, want_u) and nc.same(got_m, want_m) and nc.same(got_e, want_e)
  shape, (indptr, indices, vals), marks = nc.special_tile(dtype)
  rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
  for k in ('nan', 'inf'):
    assert not np.isfinite(got_u[rows[marks[k]]]).any() and not np.isfinite(got_m[indices[marks[k]]]).any()
  # the half that shares no row and no column with them: byte for byte, the zero rating included
  assert got_u[6:].tobytes() == want_u[6:].tobytes() and got_m[40:].tobytes() == want_m[40:].tobytes()
  assert got_e[marks['zero']] == want_e[marks['zero']] > 0.1


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_a_second_pass_and_a_repeated_call(be, dtype):
  """Two epochs: a second call on the first call's output, with the tile's plan reused; and the first call again on
  fresh operands gives the same bits."""
  name, f = 'pairs and their successors', 17
  shape, (indptr, indices, vals) = nc.cases(dtype, _hip.SP_MF_WIDE)[name]
  u1, m1, _, _, (t, ud, md) = _run(be, name, f, dtype)
  plan = t._mf_plan
  assert plan is not None
  be.sgd_mf(t, ud[:, :f], md[:, :f])
  assert t._mf_plan is plan
  want_u, want_m, _ = nc.restated(indptr, indices, vals, *_want(name, f, dtype)[:2])
  assert ud.numpy()[:, :f].tobytes() == want_u.tobytes() and md.numpy()[:, :f].tobytes() == want_m.tobytes()
  again_u, again_m, _, _, _ = _run(be, name, f, dtype)
  assert again_u.tobytes() == u1.tobytes() and again_m.tobytes() == m1.tobytes()


def test_lr_and_the_launcher(be):
  dt = np.dtype(np.float32)
  shape, (indptr, indices, vals) = nc.cases(dt, _hip.SP_MF_WIDE)['narrow wide narrow']
  u0, m0 = nc.factors(shape[0], shape[1], 7, dt)
  want_u, want_m, want_e = nc.restated(indptr, indices, vals, u0, m0, lr=0.01)
  t = _tile(be, shape, indptr, indices, vals)
  host, dev = sparse_mod.sgd_mf_plan(t)
  ud, md, err = be.from_numpy(np.ascontiguousarray(u0)), be.from_numpy(np.ascontiguousarray(m0)), be.empty((len(indices),), dt)
  launched = kernels.sgd_mf(shape, t.data, dev, host, ud, md, 0.01, abs_err=err)
  assert launched == len(kernels.sgd_mf_plan_parts(host)['segments']) == 3
  assert ud.numpy().tobytes() == want_u.tobytes() and md.numpy().tobytes() == want_m.tobytes()
  assert err.numpy().tobytes() == want_e.tobytes()


def test_refusals_launch_nothing(be):
  f32 = np.dtype(np.float32)
  shape, (indptr, indices, vals) = nc.cases(f32, _hip.SP_MF_WIDE)['dense 8 x 8']
  u0, m0 = nc.factors(8, 8, 5, f32)
  dev = lambda v: be.from_numpy(np.ascontiguousarray(v))   # noqa: E731
  t = _tile(be, shape, indptr, indices, vals)
  host, plan = sparse_mod.sgd_mf_plan(t)
  ud, md = dev(u0), dev(m0)
  big = _hip.SP_MF_MAX_F + 1
  cases = [
      (TypeError, 'astype', dict(u=dev(u0.astype(np.float64)))),
      (TypeError, 'astype', dict(m=dev(m0.astype(np.int32)))),
      (ValueError, 'U of shape', dict(u=dev(u0[:7]))),
      (ValueError, 'M of shape', dict(m=dev(m0[:, :4]))),
      (ValueError, 'rank f = %d' % big, dict(u=dev(np.zeros((8, big), f32)), m=dev(np.zeros((8, big), f32)))),
      (ValueError, 'lr', dict(lr=float('nan'))),
      (ValueError, 'lr', dict(lr=float('inf'))),
  ]
  for exc, match, change in cases:
    kw = dict(u=ud, m=md, lr=None)
    kw.update(change)
    with pytest.raises(exc, match=match):                     # the check itself, the backend and the launcher alike
      tile_checks.check_sgd_mf([f32, be.dtype_of(kw['u']), be.dtype_of(kw['m'])], shape, kw['u'].shape, kw['m'].shape, kw['lr'])
    before = be.launches
    with pytest.raises(exc, match=match):
      be.sgd_mf(t, kw['u'], kw['m'], lr=kw['lr'])
    with pytest.raises(exc, match=match):
      kernels.sgd_mf(shape, t.data, plan, host, kw['u'], kw['m'], kw['lr'])
    assert be.launches == before
  with pytest.raises(TypeError, match='sparse tile'):
    be.sgd_mf(dev(np.zeros((8, 8), f32)), ud, md)
  with pytest.raises(ValueError, match='abs_err'):
    kernels.sgd_mf(shape, t.data, plan, host, ud, md, abs_err=be.empty((3,), f32))
  with pytest.raises(ValueError, match='in place'):
    be.sgd_mf(t, dev(u0.T.copy()).t(), md)
  # the library's own refusals: a plan of another tile, a leading dimension below f, NULL operands
  lib = _hip.extras()
  p = lambda a: a.data_ptr()   # noqa: E731
  other = kernels.sgd_mf_plan(8, 9, indptr, indices)
  assert lib.sp_sgd_mf(_hip.SP_F32, 8, 8, 5, 64, p(t.data), p(plan), other.ctypes.data, p(ud), 5, p(md), 5, 1e-5, None, None, None) != 0
  assert lib.sp_sgd_mf(_hip.SP_F32, 8, 8, 5, 64, p(t.data), p(plan), host.ctypes.data, p(ud), 4, p(md), 5, 1e-5, None, None, None) != 0
  assert lib.sp_sgd_mf(_hip.SP_F32, 8, 8, 5, 64, p(t.data), p(plan), host.ctypes.data, None, 5, p(md), 5, 1e-5, None, None, None) != 0
  assert ud.numpy().tobytes() == u0.tobytes() and md.numpy().tobytes() == m0.tobytes()       # nothing was launched
