"""sp_fuzzy_step (csrc/fuzzy.hip) through HipBackend.fuzzy_step and kernels.fuzzy_step, against the oracle, the recipe
and the derived bound of tests/fuzzy_cases.py.

Shapes, for the tiling that was built (include/spartan_hip_fuzzy.h): a workgroup owns 64 rows, so n is 1 and on both
sides of 64 and 128; the centres pass 64 at a time, four to a thread, and the row's sum and arg-max run over the 16
lanes of a row, so k is 1, 2 (one lane), 5 (two lanes), on both sides of 64 and 128; the features come in chunks of 16
(d = 0, 1, 15, 16, 17) and the accumulation in panels of 128 (d = 127, 128, 129, and 257: three panels); (600, 5, 20) has
ten row blocks, (70, 300, 33) five centre blocks.  Nothing is larger than 600 x 300 x 300.  Every call of a few rows is
one range; the ranges and their combine kernel are the subject of the `splits` test.  Measured figures are printed
before each assertion (pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, kernels
from tests import fuzzy_cases as fc

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
# (n, k, d): a chosen list
SHAPES = (
    (1, 1, 1), (5, 2, 0), (63, 2, 15), (64, 63, 16), (65, 64, 17), (130, 65, 0), (5, 129, 1), (130, 129, 20), (127, 5, 3),
    (128, 128, 5), (129, 127, 16), (33, 7, 127), (64, 3, 128), (65, 5, 129), (70, 64, 257), (600, 5, 20), (70, 300, 33),
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


def _step(be, x, c, m, want_u=True, splits=0):
  """The outputs of one backend call on host operands, as host arrays."""
  out = be.fuzzy_step(be.from_numpy(np.ascontiguousarray(x)), be.from_numpy(np.ascontiguousarray(c)), m, want_u=want_u,
                      splits=splits)
  return tuple(t.numpy() for t in out)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('m', fc.MS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_every_output_meets_the_derived_bound(be, shape, m, dtype):
  n, k, d = shape
  x, c = fc.case(n, k, d, np.dtype(dtype))
  want = fc.oracle_of_case(n, k, d, np.dtype(dtype), m)
  xt, ct = be.from_numpy(x), be.from_numpy(c)
  before = be.launches
  with_u = be.fuzzy_step(xt, ct, m, want_u=True)
  without = be.fuzzy_step(xt, ct, m)
  assert be.launches - before == 2          # (one per call: HipBackend.fuzzy_step's docstring)
  assert len(with_u) == 4 and len(without) == 3
  labels, sums, wsum, u = (t.numpy() for t in with_u)
  name = 'hip %s m=%g %s' % (shape, m, np.dtype(dtype).name)
  fc.check_step(x, c, m, labels, sums, wsum, u, want=want, label=name)
  for a, b in zip(without, (labels, sums, wsum)):       # U is an extra output, nothing else
    assert a.numpy().tobytes() == b.tobytes()
  if n > 3 and d > 0:
    assert np.all(np.isfinite(u)) and np.all(u > 0)     # centre 0 == point 3: the 1e-10 path
    tiny = float(np.dtype(dtype).type(1e-10))
    p = tiny if m == 2.0 else tiny ** float(np.dtype(dtype).type(1.0 / (m - 1.0)))
    assert abs(float(u[3, 0]) - p / float(want['z'][3])) <= fc.eps(n, k, d, m, dtype)['u'] * p / float(want['z'][3])
  if k >= 3 and n:
    assert not np.any(labels == k - 1)                  # the last centre duplicates centre 1: the lower index wins
  if d == 0 and n:
    assert np.all(np.abs(u - 1.0 / k) <= fc.eps(n, k, d, m, dtype)['u'] / k) and not np.any(labels)      # u = 1 / k
  assert xt.numpy().tobytes() == x.tobytes() and ct.numpy().tobytes() == c.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('m', (2.0, 1.5))
def test_splits_change_no_label_and_no_membership(be, m, dtype):
  n, k, d = 300, 70, 20
  x, c = fc.case(n, k, d, np.dtype(dtype))
  want = fc.oracle_of_case(n, k, d, np.dtype(dtype), m)
  base = _step(be, x, c, m, splits=0)
  seen = {}
  for s in (0, 1, 2, 3, 7):
    labels, sums, wsum, u = _step(be, x, c, m, splits=s)
    fc.check_step(x, c, m, labels, sums, wsum, u, want=want, label='hip splits=%d m=%g %s' % (s, m, np.dtype(dtype).name))
    assert labels.tobytes() == base[0].tobytes() and u.tobytes() == base[3].tobytes()
    again = _step(be, x, c, m, splits=s)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (labels, sums, wsum, u)))
    seen[s] = sums.tobytes() + wsum.tobytes()
  assert seen[0] == seen[1]                 # five row blocks: the library does not cut them
  assert seen[7] != seen[1] and seen[2] != seen[1]      # another order of the same rows (300 rows, 70 x 20 sums)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('m', (2.0, 3.0))
def test_a_row_depends_on_itself_and_the_centres_alone(be, m, dtype):
  n, k, d = 70, 67, 20
  x, c = fc.case(n, k, d, np.dtype(dtype), seed=2)
  labels, sums, wsum, u = _step(be, x, c, m)
  for i in (0, 3, 63, 64, 69):                          # alone: another place in the workgroup, no neighbours
    li, _, _, ui = _step(be, x[i:i + 1], c, m)
    assert li.tobytes() == labels[i:i + 1].tobytes() and ui.tobytes() == u[i:i + 1].tobytes(), i
  lb, sb, wb, ub = _step(be, x[::-1], c, m)
  assert lb[::-1].tobytes() == labels.tobytes() and ub[::-1].tobytes() == u.tobytes()
  fc.check_step(np.ascontiguousarray(x[::-1]), c, m, lb, sb, wb, ub, label='hip rows reversed')
  changed = np.array(x)
  changed[4] = changed[4][::-1] * 0.5
  lc, sc, wc, uc = _step(be, changed, c, m)
  assert np.delete(uc, 4, axis=0).tobytes() == np.delete(u, 4, axis=0).tobytes()
  assert np.delete(lc, 4).tobytes() == np.delete(labels, 4).tobytes()
  assert uc[4].tobytes() != u[4].tobytes() and sc.tobytes() != sums.tobytes() and wc.tobytes() != wsum.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', ((70, 67, 20), (65, 5, 129)), ids=lambda s: '%dx%dx%d' % s)
def test_views_of_wider_buffers_give_the_same_bits(be, shape, dtype):
  n, k, d = shape
  m = 1.5
  x, c = fc.case(n, k, d, np.dtype(dtype), seed=1)
  labels, sums, wsum, u = _step(be, x, c, m)
  (xt, xbuf, xframe), (ct, cbuf, cframe) = _framed(be, x, 3), _framed(be, c, 5)
  (st, sbuf, sframe), (ut, ubuf, uframe) = _framed(be, np.zeros((k, d), dtype), 7), _framed(be, np.zeros((n, k), dtype), 2)
  lt, wt = be.empty((n,), np.int64), be.empty((k,), dtype)
  kernels.fuzzy_step(xt, ct, m, lt, st, wt, u=ut)
  assert lt.numpy().tobytes() == labels.tobytes() and wt.numpy().tobytes() == wsum.tobytes()
  assert st.numpy().tobytes() == sums.tobytes() and ut.numpy().tobytes() == u.tobytes()
  assert xbuf.numpy().tobytes() == xframe.tobytes() and cbuf.numpy().tobytes() == cframe.tobytes()
  sframe[1:k + 1, 1:d + 1] = sums
  uframe[1:n + 1, 1:k + 1] = u
  assert sbuf.numpy().tobytes() == sframe.tobytes() and ubuf.numpy().tobytes() == uframe.tobytes()     # frames untouched
  # without labels and without U
  st2, wt2 = be.empty((k, d), dtype), be.empty((k,), dtype)
  kernels.fuzzy_step(xt, ct, m, None, st2, wt2)
  assert st2.numpy().tobytes() == sums.tobytes() and wt2.numpy().tobytes() == wsum.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_duplicate_centres_and_a_nan_row(be, dtype):
  n, k, d = 70, 6, 9
  m = 2.0
  x, c = fc.case(n, k, d, np.dtype(dtype), seed=3)
  labels, sums, wsum, u = _step(be, x, c, m)
  far = int(labels[0])
  behind = np.vstack([c, c[far:far + 1]])                # a copy of row 0's farthest centre at a HIGHER index: no change
  assert _step(be, x, behind, m)[0].tobytes() == labels.tobytes()
  ahead = np.vstack([c[far:far + 1], c])                 # ... at index 0: it takes every label the original had
  got = _step(be, x, ahead, m)[0]
  assert got.tobytes() == np.where(labels == far, 0, labels + 1).tobytes()
  bad = np.array(x)
  bad[5, d // 2] = np.nan
  ln, sn, wn, un = _step(be, bad, c, m)
  assert ln[5] == 0                                      # every distance of the row is NaN: the first one
  assert np.all(np.isnan(un[5])) and np.all(np.isnan(sn)) and np.all(np.isnan(wn))
  assert np.delete(un, 5, axis=0).tobytes() == np.delete(u, 5, axis=0).tobytes()
  assert np.delete(ln, 5).tobytes() == np.delete(labels, 5).tobytes()
  nan_centre = np.array(c)
  nan_centre[2, 0] = np.nan                              # one NaN distance per row, at centre 2
  ln = _step(be, x, nan_centre, m)[0]
  assert np.all(ln == 2)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_empty_inputs(be, dtype):
  labels, sums, wsum, u = _step(be, np.zeros((0, 6), dtype), np.ones((4, 6), dtype), 2.0)
  assert labels.shape == (0,) and u.shape == (0, 4) and sums.shape == (4, 6) and wsum.shape == (4,)
  assert not np.any(sums) and not np.any(wsum)
  x = np.ones((66, 0), dtype)
  labels, sums, wsum, u = _step(be, x, np.ones((3, 0), dtype), 1.5)
  assert sums.shape == (3, 0) and not np.any(labels)
  assert np.all(np.abs(u - 1.0 / 3) <= fc.eps(66, 3, 0, 1.5, dtype)['u'] / 3)           # u = 1 / k within the bound
  fc.check_step(x, np.ones((3, 0), dtype), 1.5, labels, sums, wsum, u, label='hip d = 0 %s' % np.dtype(dtype).name)


def test_refusals_launch_nothing(be):
  x, c = fc.case(9, 4, 3, np.dtype(np.float32))
  xt, ct = be.from_numpy(x), be.from_numpy(c)
  before = be.launches
  for bad_x, bad_c in ((x.astype(np.int32), c.astype(np.int32)), (x.astype(np.float16), c.astype(np.float16)),
                       (x, c.astype(np.float64)), (x.astype(np.int32), c)):
    with pytest.raises(TypeError, match='astype'):
      be.fuzzy_step(be.from_numpy(bad_x), be.from_numpy(bad_c), 2.0)
  for m in (1.0, 0.5, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='m = '):
      be.fuzzy_step(xt, ct, m)
  with pytest.raises(ValueError, match='k = 0'):
    be.fuzzy_step(xt, be.from_numpy(np.zeros((0, 3), np.float32)), 2.0)
  with pytest.raises(ValueError, match='fit'):
    be.fuzzy_step(xt, be.from_numpy(np.zeros((4, 2), np.float32)), 2.0)
  labels, sums, wsum = be.empty((9,), np.int64), be.empty((4, 3), np.float32), be.empty((4,), np.float32)
  with pytest.raises(TypeError, match='astype'):
    kernels.fuzzy_step(xt, be.from_numpy(c.astype(np.float64)), 2.0, labels, sums, wsum)
  with pytest.raises(TypeError, match='astype'):
    kernels.fuzzy_step(xt, ct, 2.0, labels, be.empty((4, 3), np.float64), wsum)
  with pytest.raises(ValueError, match='m = '):
    kernels.fuzzy_step(xt, ct, 1.0, labels, sums, wsum)
  for bad in (dict(sums=be.empty((4, 4), np.float32)), dict(wsum=be.empty((5,), np.float32)),
              dict(labels=be.empty((8,), np.int64)), dict(u=be.empty((9, 5), np.float32))):
    args = dict(labels=labels, sums=sums, wsum=wsum, u=None)
    args.update(bad)
    with pytest.raises(ValueError):
      kernels.fuzzy_step(xt, ct, 2.0, args['labels'], args['sums'], args['wsum'], u=args['u'])
  assert be.launches == before
  # the library's own refusals
  lib, err = _hip.extras(), _hip.lib().sp_last_error
  f32 = _hip.SP_F32
  assert lib.sp_fuzzy_step(_hip.SP_I32, None, 3, 9, None, 3, 4, 3, 2.0, 0, None, None, 3, None, None, 4, None, 0, None) != 0
  assert 'astype' in err().decode()
  assert lib.sp_fuzzy_step(_hip.SP_F16, None, 3, 9, None, 3, 4, 3, 2.0, 0, None, None, 3, None, None, 4, None, 0, None) != 0
  assert 'astype' in err().decode()
  for m in (1.0, 0.5, float('nan'), float('inf')):
    assert lib.sp_fuzzy_step(f32, None, 3, 9, None, 3, 4, 3, m, 0, None, None, 3, None, None, 4, None, 0, None) != 0
    assert 'm = ' in err().decode()
  assert lib.sp_fuzzy_step(f32, None, 3, 9, None, 3, 0, 3, 2.0, 0, None, None, 3, None, None, 4, None, 0, None) != 0
  assert 'k = 0' in err().decode()
  assert lib.sp_fuzzy_step(f32, None, 2, 9, None, 3, 4, 3, 2.0, 0, None, None, 3, None, None, 4, None, 0, None) != 0
  assert 'bad shape' in err().decode()
  assert lib.sp_fuzzy_step(f32, None, 3, 9, None, 3, 4, 3, 2.0, 0, None, None, 3, None, None, 4, None, 0, None) != 0
  assert 'required' in err().decode()                    # (no targets: refused before the workspace is looked at)
