"""sp_als_solve (csrc/als.hip) through HipBackend.als_solve and kernels.als_solve, against the oracle and the derived
bound of tests/als_cases.py.

Shapes: a workgroup owns 4 rows of R (one per wave) and streams the items through LDS 64 at a time, so m is 1 and on
both sides of 4 and 8, n is 0, 1 and on both sides of 64 and 128; implicit mode's pre-pass cuts the items into ranges of
256, so n is on both sides of 256 as well; 1031 and 2049 are the long rows.  The switch between the two register
layouts is at f = 32 / 33 (4 x 4 blocks of A_i up to 32, 8 x 8 above); within the first layout the number of items a
wave takes at once changes with the number of blocks (f <= 4: 64, 8: 21, 20: 4, 21 .. 32: 2 or 1), hence f = 1, 2, 3, 8,
20, 21, 32, 33, 63, 64.  With f near 64 an implicit
system of few items is too ill-conditioned for the float32 bound to say anything (kappa eA >= 1: als_cases rejects it),
so those f come with n >= 300 and the chunk edges of the second layout with f = 33.  Nothing is larger than 130 x 2100.  Measured figures are printed before each assertion
(pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, kernels
from tests import als_cases as ac

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
MODES = (False, True)
# (m, n, f): a chosen list
SHAPES = (
    (1, 0, 3), (5, 0, 20), (1, 1, 1), (3, 1, 3), (4, 63, 2), (5, 64, 3), (7, 65, 8), (8, 127, 20), (9, 128, 21),
    (3, 129, 32), (4, 257, 33), (5, 310, 63), (4, 300, 64), (6, 255, 1), (2, 256, 8), (9, 129, 33), (5, 320, 64), (4, 1031, 20),
    (3, 2049, 33), (130, 70, 20),
)


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _framed(be, a, pad, fill=-77.0):
  """`a` as a row view of a wider device array (row stride a.shape[1] + pad): (view, the whole buffer, its host image)."""
  frame = np.full((a.shape[0] + 2, a.shape[1] + pad), fill, a.dtype)
  frame[1:a.shape[0] + 1, 1:a.shape[1] + 1] = a
  buf = be.from_numpy(frame)
  return buf[1:a.shape[0] + 1, 1:a.shape[1] + 1], buf, frame


def _name(implicit):
  return 'implicit' if implicit else 'explicit'


def _solve(be, r, y, implicit, la=ac.LA, alpha=ac.ALPHA):
  """(x on the host, info) of one backend call on host operands."""
  info = be.zeros((1,), np.int32)
  x = be.als_solve(be.from_numpy(np.ascontiguousarray(r)), be.from_numpy(np.ascontiguousarray(y)), la, alpha,
                   implicit=implicit, info=info)
  return x.numpy(), int(info.numpy()[0])


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('implicit', MODES, ids=_name)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_every_row_meets_the_derived_bound(be, shape, implicit, dtype):
  m, n, f = shape
  r, y = ac.case(m, n, f, dtype)
  want, bound, _ = ac.oracle_of_case(m, n, f, dtype, implicit)
  rt, yt, info = be.from_numpy(r), be.from_numpy(y), be.zeros((1,), np.int32)
  before = be.launches
  x = be.als_solve(rt, yt, ac.LA, ac.ALPHA, implicit=implicit, info=info)
  assert be.launches - before == 1          # (m > 0 in every case: HipBackend.als_solve's docstring)
  got = x.numpy()
  assert got.dtype == np.dtype(dtype) and got.shape == (m, f)
  ac.check(got, want, bound, 'hip %s %s %s' % (shape, np.dtype(dtype).name, _name(implicit)))
  if m > 1 and not implicit:
    assert not np.any(got[1])               # nothing rated: exactly 0
  if n == 0:
    assert not np.any(got)
  assert int(info.numpy()[0]) == 0
  assert rt.numpy().tobytes() == r.tobytes() and yt.numpy().tobytes() == y.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('implicit', MODES, ids=_name)
def test_negative_ratings_in_explicit_mode_and_no_rows(be, implicit, dtype):
  empty = be.als_solve(be.from_numpy(np.zeros((0, 9), dtype)), be.from_numpy(np.zeros((9, 5), dtype)), ac.LA, ac.ALPHA,
                       implicit=implicit)
  assert tuple(empty.shape) == (0, 5)
  if not implicit:
    r, y = ac.case(6, 70, 5, dtype, negative=True)
    want, bound, _ = ac.oracle_of_case(6, 70, 5, dtype, False, negative=True)
    got, info = _solve(be, r, y, False)
    ac.check(got, want, bound, 'hip negative ratings %s' % np.dtype(dtype).name)
    assert info == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('implicit', MODES, ids=_name)
@pytest.mark.parametrize('shape', ((5, 129, 20), (6, 70, 33)), ids=lambda s: '%dx%dx%d' % s)
def test_views_of_wider_buffers_give_the_same_bits(be, shape, implicit, dtype):
  m, n, f = shape
  r, y = ac.case(m, n, f, dtype, seed=1)
  dense, _ = _solve(be, r, y, implicit)
  (rt, rbuf, rframe), (yt, ybuf, yframe) = _framed(be, r, 3), _framed(be, y, 5)
  xt, xbuf, xframe = _framed(be, np.zeros((m, f), dtype), 7)
  info = be.zeros((1,), np.int32)
  kernels.als_solve(rt, yt, ac.LA, ac.ALPHA, implicit, xt, info)
  assert xt.numpy().tobytes() == dense.tobytes()
  assert rbuf.numpy().tobytes() == rframe.tobytes() and ybuf.numpy().tobytes() == yframe.tobytes()
  after = xbuf.numpy()
  xframe[1:m + 1, 1:f + 1] = dense
  assert after.tobytes() == xframe.tobytes()          # the frame around the target: untouched
  assert int(info.numpy()[0]) == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('implicit', MODES, ids=_name)
@pytest.mark.parametrize('shape', ((9, 130, 20), (6, 200, 3), (7, 70, 64)), ids=lambda s: '%dx%dx%d' % s)
def test_a_row_depends_on_its_own_ratings_alone(be, shape, implicit, dtype):
  m, n, f = shape
  r, y = ac.case(m, n, f, dtype, seed=2)
  whole, _ = _solve(be, r, y, implicit)
  for i in range(m):                                   # alone: another place in the workgroup, no neighbours
    alone, _ = _solve(be, r[i:i + 1], y, implicit)
    assert alone.tobytes() == whole[i:i + 1].tobytes(), i
  backwards, _ = _solve(be, r[::-1], y, implicit)
  assert backwards[::-1].tobytes() == whole.tobytes()
  changed = np.array(r)
  changed[4, n // 3] = 1 if changed[4, n // 3] != 1 else 2
  other, _ = _solve(be, changed, y, implicit)
  assert np.delete(other, 4, axis=0).tobytes() == np.delete(whole, 4, axis=0).tobytes()
  assert other[4].tobytes() != whole[4].tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('f', (5, 40))
def test_an_indefinite_system_fails_its_row_alone(be, f, dtype):
  """One strongly negative rating makes one row's implicit system indefinite; a NaN rating does the same.  An
  arithmetic outcome: the row is NaN, info names it, every other row keeps its bits."""
  m, n = 11, 40
  r, y = ac.case(m, n, f, dtype, seed=3)
  clean, info = _solve(be, r, y, True)
  assert info == 0 and np.all(np.isfinite(clean))
  for poison in (-500.0, np.nan):
    bad = np.array(r)
    bad[6, 7] = poison
    got, info = _solve(be, bad, y, True)
    assert info == 7
    assert np.all(np.isnan(got[6]))
    assert np.delete(got, 6, axis=0).tobytes() == np.delete(clean, 6, axis=0).tobytes()
  two = np.array(r)
  two[9, 3] = two[5, 3] = -500.0                        # two failing rows: the lowest is reported
  got, info = _solve(be, two, y, True)
  assert info == 6 and np.all(np.isnan(got[[5, 9]])) and np.all(np.isfinite(np.delete(got, [5, 9], axis=0)))
  # a word that is already set is left alone
  word = be.from_numpy(np.array([3], np.int32))
  be.als_solve(be.from_numpy(two), be.from_numpy(y), ac.LA, ac.ALPHA, implicit=True, info=word)
  assert int(word.numpy()[0]) == 3
  nan_explicit = np.array(r)
  nan_explicit[2, 5] = np.nan
  got, info = _solve(be, nan_explicit, y, False)
  assert info == 3 and np.all(np.isnan(got[2])) and np.all(np.isfinite(np.delete(got, 2, axis=0)))


def test_refusals_launch_nothing(be):
  r, y = ac.case(4, 9, 3, np.float32)
  rt, yt = be.from_numpy(r), be.from_numpy(y)
  before = be.launches
  for bad_r, bad_y in ((r.astype(np.int32), y.astype(np.int32)), (r.astype(np.float16), y.astype(np.float16)),
                       (r, y.astype(np.float64)), (r.astype(np.int32), y)):
    with pytest.raises(TypeError, match='astype'):
      be.als_solve(be.from_numpy(bad_r), be.from_numpy(bad_y), ac.LA, ac.ALPHA)
  for f in (0, 65):
    with pytest.raises(ValueError, match='64'):
      be.als_solve(rt, be.from_numpy(np.zeros((9, f), np.float32)), ac.LA, ac.ALPHA)
  with pytest.raises(ValueError, match='fit'):
    be.als_solve(rt, be.from_numpy(np.zeros((8, 3), np.float32)), ac.LA, ac.ALPHA)
  x, info = be.empty((4, 3), np.float32), be.zeros((1,), np.int32)
  with pytest.raises(TypeError, match='astype'):
    kernels.als_solve(rt, be.from_numpy(y.astype(np.float64)), ac.LA, ac.ALPHA, False, x, info)
  with pytest.raises(ValueError, match='64'):
    kernels.als_solve(rt, be.from_numpy(np.zeros((9, 65), np.float32)), ac.LA, ac.ALPHA, False, x, info)
  with pytest.raises(ValueError):
    kernels.als_solve(rt, yt, ac.LA, ac.ALPHA, False, be.empty((4, 4), np.float32), info)
  assert be.launches == before
  # the library's own refusals, with the limit by name
  lib = _hip.extras()
  assert lib.sp_als_solve(_hip.SP_F32, None, 9, 4, 9, None, 65, 65, 0.1, 1.0, 0, None, 65, None, None, 0, None) != 0
  assert '64' in _hip.lib().sp_last_error().decode()
  assert lib.sp_als_solve(_hip.SP_I32, None, 9, 4, 9, None, 3, 3, 0.1, 1.0, 0, None, 3, None, None, 0, None) != 0
  assert 'astype' in _hip.lib().sp_last_error().decode()
