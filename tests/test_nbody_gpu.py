"""sp_nbody_accel (csrc/nbody.hip) through HipBackend.nbody_accel and kernels.nbody_accel, against the oracle, the
derived bound and the rebuilt order of tests/nbody_cases.py, and the n-body driver on the device.

Bodies: n = 1, 2, 3, 63, 64, 65, 130, 257 and 600, for the tiling that was built (include/spartan_hip_nbody.h): a block
is 64 sources and a workgroup 64 targets, so n sits on both sides of 64 and of 128 and 256, and 600 is ten blocks with a
padded last one; under splits = 0 the sources are cut into 2, 3, 5 and 10 ranges at 65, 130, 257 and 600.  Nothing is
larger.  Unit-scale cases (g = 1, rmin = 0.05).  Measured shares of the bound are printed before each assertion
(pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, devarray, kernels
from spartan_amd.examples import _nbody
from tests import nbody_cases as nc
from tests import test_nbody_example as ex

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
SIZES = (1, 2, 3, 63, 64, 65, 130, 257, 600)
G, RMIN = nc.UNIT_G, nc.UNIT_RMIN
dtype_ids = dict(ids=lambda d: np.dtype(d).name)


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _accel(be, x, y, z, mass, r0=0, m=None, g=G, rmin=RMIN, splits=0):
  m = len(x) - r0 if m is None else m
  out = be.nbody_accel(*(be.from_numpy(np.ascontiguousarray(v)) for v in (x, y, z, mass)), r0, m, g=g, rmin=rmin,
                       splits=splits)
  return tuple(t.numpy() for t in out)


def _same(a, b):
  return all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('n', SIZES)
def test_every_output_meets_the_derived_bound(be, n, dtype):
  dt = np.dtype(dtype)
  case = nc.unit_case(n, dt, kind='placed' if n >= 63 else 'random')
  before = be.launches
  got = _accel(be, *case)
  assert be.launches - before == (1 if nc.ranges_of(n, 0) == 1 else 2)
  assert all(v.dtype == dt and v.shape == (n,) for v in got)
  if n == 1:
    assert not any(v.any() for v in got)                       # n = 1: zeros
  else:
    nc.check_accel(got, *case, G, RMIN, 'hip n=%d %s' % (n, dt.name))
  assert _same(_accel(be, *case), got)                         # a repeated call: the same bits


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_one_pair_is_the_term_bit_for_bit(be, dtype):
  """n = 2: a[j] = (0 + t) + (0 + 0) = the one term -- IEEE sqrt and division, no contraction."""
  dt = np.dtype(dtype)
  for seed in range(4):
    x, y, z, mass = nc.unit_case(2, dt, seed=seed)
    got = _accel(be, x, y, z, mass)
    for j in (0, 1):
      for k, t in enumerate(_nbody.pair_terms(x, y, z, mass, j, G, RMIN)):
        assert t[1 - j] != 0 and got[k][j].tobytes() == t[1 - j].tobytes(), (seed, j, k)
  # the golden galaxy's first pair in SI units (float64: r^3 is about 1e42)
  if dt == np.float64:
    start = nc.golden_input()
    x, y, z, mass = (np.array(start[k][:2]) for k in ('x', 'y', 'z', 'm'))
    got = _accel(be, x, y, z, mass, g=nc.G, rmin=1.0)
    for k, t in enumerate(_nbody.pair_terms(x, y, z, mass, 0, nc.G, 1.0)):
      assert got[k][0].tobytes() == t[1].tobytes()


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('n', (130, 257, 600))
def test_the_sum_is_added_in_the_stated_order(be, n, dtype):
  dt = np.dtype(dtype)
  case = nc.unit_case(n, dt, kind='placed')
  targets = sorted(set(list(range(0, n, 37)) + [1, 3, 63, 64, 65, n - 2, n - 1, n // 2 + 1]))
  for splits in (0, 1, 2, 3, 64):
    got = _accel(be, *case, splits=splits)
    want = nc.ordered_accel(*case, G, RMIN, splits, targets)
    for k in range(3):
      assert got[k][targets].tobytes() == want[k].tobytes(), (splits, k)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_split_arithmetic(be, dtype):
  """splits = 2 and 3: the ranges' own sums -- each range's sources alone, the other sources given mass 0 so that
  their terms are +0 -- added in ascending range order."""
  dt = np.dtype(dtype)
  n = 257
  x, y, z, mass = nc.unit_case(n, dt)
  nb = -(-n // 64)
  for splits in (2, 3):
    got = _accel(be, x, y, z, mass, splits=splits)
    cuts = [(g * nb // splits) * 64 for g in range(splits)] + [n]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
      only = np.zeros_like(mass)
      only[lo:hi] = mass[lo:hi]
      parts.append(_accel(be, x, y, z, only, splits=1))
    for k in range(3):
      acc = parts[0][k]
      for p in parts[1:]:
        acc = acc + p[k]
      assert got[k].tobytes() == acc.tobytes(), (splits, k)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('n', (130, 600))
def test_a_band_gives_the_bits_of_the_whole(be, n, dtype):
  case = nc.unit_case(n, np.dtype(dtype), kind='placed')
  for splits in (0, 1):
    whole = _accel(be, *case, splits=splits)
    for r0, m in ((0, n), (5, 9), (64, 64), (n - 1, 1), (63, 2)):
      band = _accel(be, *case, r0=r0, m=m, splits=splits)
      assert all(v.shape == (m,) for v in band)
      assert _same(band, [w[r0:r0 + m] for w in whole]), (splits, r0, m)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_neighbours(be, dtype):
  dt = np.dtype(dtype)
  n = 257
  x, y, z, mass = (np.array(v) for v in nc.unit_case(n, dt))
  base = _accel(be, x, y, z, mass, splits=1)
  j, k = 70, 133                                   # (k mod 4 = 1: class 1 of block 2)
  moved = x.copy()
  moved[k] = x[k] + dt.type(0.25) if x[k] < 0.5 else x[k] - dt.type(0.25)
  nc.assert_clear_of_rmin(moved, y, z, RMIN)
  got = _accel(be, moved, y, z, mass, splits=1)
  # body k changed: a[j] is the stated sum of the new terms, where only term k differs
  old_terms = _nbody.pair_terms(x, y, z, mass, j, G, RMIN)
  new_terms = _nbody.pair_terms(moved, y, z, mass, j, G, RMIN)
  for c in range(3):
    differ = np.flatnonzero(old_terms[c] != new_terms[c])
    assert set(differ.tolist()) <= {k}
    assert got[c][j].tobytes() == nc.ordered_sum(new_terms[c], n, 1).tobytes()
  # two far sources of one position class swapped (130 and 194: both i mod 4 = 2, blocks 2 and 3): within the bound;
  # the order of a[j]'s terms has changed, so its bits may
  perm = np.arange(n)
  perm[[130, 194]] = [194, 130]
  swapped = _accel(be, x[perm], y[perm], z[perm], mass[perm], splits=1)
  nc.check_accel(swapped, x[perm], y[perm], z[perm], mass[perm], G, RMIN, 'hip swapped sources %s' % dt.name)
  inv = [v[perm] for v in swapped]                 # (the permutation is its own inverse)
  want = nc.oracle(x, y, z, mass, G, RMIN)
  nc.check_accel(inv, x, y, z, mass, G, RMIN, 'hip swapped sources, back in place %s' % dt.name, want=want)
  nc.check_accel(base, x, y, z, mass, G, RMIN, 'hip base %s' % dt.name, want=want)


@pytest.mark.parametrize('splits', (1, 0))
@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_launches(be, dtype, splits):
  case = nc.unit_case(130, np.dtype(dtype))
  before = be.launches
  _accel(be, *case, splits=splits)
  assert be.launches - before == (1 if splits == 1 else 2)      # one range: one kernel; more: the partial sum as well
  before = be.launches
  _accel(be, *case, r0=7, m=0)
  assert be.launches == before                                  # m = 0 launches nothing


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_special_values(be, dtype):
  dt = np.dtype(dtype)
  n = 130
  x, y, z, mass = (np.array(v) for v in nc.unit_case(n, dt, kind='placed'))
  (a, b), (c, d) = nc.placed_pairs(n)
  rmin = dt.type(RMIN)
  for splits in (1, 0):
    got = _accel(be, x, y, z, mass, splits=splits)
    nc.check_accel(got, x, y, z, mass, G, RMIN, 'hip placed pairs %s splits=%d' % (dt.name, splits))
    # the coincident pair contributes exactly 0: without body d in the sum, a[c] has the same bits
    gone = mass.copy()
    gone[d] = 0
    assert all(p[c].tobytes() == q[c].tobytes() for p, q in zip(got, _accel(be, x, y, z, gone, splits=splits)))
    # the pair at rmin / 2 uses rmin: alone (every other mass 0) the term is (g m_b / rmin^3) dx
    only = np.zeros_like(mass)
    only[b] = mass[b]
    alone = _accel(be, x, y, z, only, splits=splits)
    w = (dt.type(G) * mass[b]) / ((rmin * rmin) * rmin)
    assert alone[0][a].tobytes() == (w * (x[b] - x[a])).tobytes() and alone[1][a] == 0 and alone[2][a] == 0
  # a body of mass 0 changes the others' sums by nothing in value: within the bound of the galaxy without it
  keep = np.arange(n) != 77
  zero = mass.copy()
  zero[77] = 0
  with_zero = _accel(be, x, y, z, zero)
  nc.check_accel([v[keep] for v in with_zero], x[keep], y[keep], z[keep], mass[keep], G, RMIN,
                 'hip a body of mass 0 %s' % dt.name)
  # NaN and inf
  bad = x.copy()
  bad[40] = np.nan
  assert all(np.isnan(v).all() for v in _accel(be, bad, y, z, mass))          # a NaN coordinate: every a is NaN
  # one infinite coordinate: r = inf, w = 0 and 0 * inf = NaN in that component for everyone; the others stay numbers
  bad[40] = np.inf
  got = _accel(be, bad, y, z, mass)
  assert np.isnan(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
  # two of them: inf - inf = NaN between the two, in every component
  bad[41] = np.inf
  got = _accel(be, bad, y, z, mass)
  others = np.ones(n, bool)
  others[[40, 41]] = False
  assert all(np.isnan(v[[40, 41]]).all() for v in got) and np.isfinite(got[1][others]).all()
  one = tuple(np.array([v], dt) for v in (np.inf, np.nan, -0.0, 1.0))
  assert not any(v.any() for v in _accel(be, *one))                           # n = 1: zeros whatever the coordinates
  # -0.0 inputs are accepted
  neg = x.copy()
  neg[5], neg[9] = -0.0, -0.0
  zneg = z.copy()
  zneg[5] = -0.0
  nc.assert_clear_of_rmin(neg, y, zneg, RMIN, nc.placed_pairs(n))
  nc.check_accel(_accel(be, neg, y, zneg, mass), neg, y, zneg, mass, G, RMIN, 'hip -0.0 inputs %s' % dt.name)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_strided_views(be, dtype):
  dt = np.dtype(dtype)
  n = 130
  case = nc.unit_case(n, dt)
  for splits in (1, 0):
    want = _accel(be, *case, splits=splits)
    frame = np.full((n + 2, 6), -77, dt)
    for c, v in enumerate(case):
      frame[1:n + 1, c + 1] = v
    buf = be.from_numpy(frame)
    views = [buf[1:n + 1, c + 1] for c in range(4)]
    assert all(v.stride(0) == 6 for v in views)
    before = be.launches
    got = be.nbody_accel(*views, 0, n, g=G, rmin=RMIN, splits=splits)
    assert be.launches - before == (1 if splits == 1 else 2)      # (the copies belong to the call)
    assert _same([t.numpy() for t in got], want)
    assert buf.numpy().tobytes() == frame.tobytes()               # inputs and frame untouched
    # the launcher writes into views of a wider target and nothing around them
    marks = np.full((5, n + 3), -5, dt)
    tgt = be.from_numpy(marks)
    dense = [be.from_numpy(np.ascontiguousarray(v)) for v in case]
    kernels.nbody_accel(*dense, 0, n, tgt[1, 2:n + 2], tgt[2, 2:n + 2], tgt[4, 2:n + 2], G, RMIN, splits=splits)
    for row, w in zip((1, 2, 4), want):
      marks[row, 2:n + 2] = w
    assert tgt.numpy().tobytes() == marks.tobytes()


def test_refusals_launch_nothing(be):
  x, y, z, mass = nc.unit_case(130, np.dtype(np.float32))
  t = [be.from_numpy(v) for v in (x, y, z, mass)]
  before = be.launches
  for bad in (np.int32, np.float16, np.int64):
    with pytest.raises(TypeError, match='astype first'):
      be.nbody_accel(t[0], be.from_numpy(y.astype(bad)), t[2], t[3], 0, 130)
  with pytest.raises(TypeError, match='two dtypes.*astype first'):
    be.nbody_accel(t[0], t[1], be.from_numpy(z.astype(np.float64)), t[3], 0, 130)
  with pytest.raises(ValueError, match='1-D and of equal length'):
    be.nbody_accel(t[0], t[1], be.from_numpy(z[:129]), t[3], 0, 129)
  with pytest.raises(ValueError, match='1-D and of equal length'):
    be.nbody_accel(*(be.from_numpy(v.reshape(130, 1)) for v in (x, y, z, mass)), 0, 130)
  for r0, m in ((-1, 2), (0, 131), (130, 1), (3, -1)):
    with pytest.raises(ValueError, match='not among'):
      be.nbody_accel(*t, r0, m)
  with pytest.raises(ValueError, match='splits'):
    be.nbody_accel(*t, 0, 130, splits=-1)
  for g in (float('nan'), float('inf'), 1e300):
    with pytest.raises(ValueError, match='g = '):
      be.nbody_accel(*t, 0, 130, g=g)
  for rmin in (0.0, -1.0, float('nan'), float('inf'), 1e-60):
    with pytest.raises(ValueError, match='rmin'):
      be.nbody_accel(*t, 0, 130, rmin=rmin)
  out = [be.empty((130,), np.float32) for _ in range(3)]
  with pytest.raises(TypeError, match='astype first'):
    kernels.nbody_accel(*t, 0, 130, out[0], be.empty((130,), np.float64), out[2], 1.0, 1.0)
  with pytest.raises(ValueError, match='targets of shapes'):
    kernels.nbody_accel(*t, 0, 130, out[0], out[1], be.empty((129,), np.float32), 1.0, 1.0)
  assert be.launches == before
  # the library's own refusals
  lib, err = _hip.extras(), _hip.lib().sp_last_error
  f32 = _hip.SP_F32
  marks = np.full((3, 130), -5, np.float32)
  tgt = be.from_numpy(marks)
  ptr = [v.data_ptr() for v in t]
  o = [tgt[c].data_ptr() for c in range(3)]
  stream = devarray.current_stream().ptr

  def call(dtype=f32, g=1.0, rmin=1.0, ins=ptr, n=130, r0=0, m=130, outs=o, splits=2, ws=None, ws_bytes=0):
    return lib.sp_nbody_accel(dtype, g, rmin, ins[0], ins[1], ins[2], ins[3], n, r0, m, outs[0], outs[1], outs[2], splits,
                              ws, ws_bytes, stream)

  for dtype in (_hip.SP_I32, _hip.SP_F16, _hip.SP_I64):
    assert call(dtype=dtype) != 0 and 'astype first' in err().decode()
  for kw in (dict(r0=-1), dict(r0=1), dict(m=131), dict(r0=131, m=0)):
    assert call(**kw) != 0 and 'not among' in err().decode()
  for kw in (dict(m=-1), dict(n=-1, m=0), dict(splits=-1)):
    assert call(**kw) != 0 and 'bad shape' in err().decode()
  for g in (float('nan'), float('inf'), 1e300):
    assert call(g=g) != 0 and 'g = ' in err().decode()
  for rmin in (0.0, -1.0, float('nan'), float('inf'), 1e-60):
    assert call(rmin=rmin) != 0 and 'rmin' in err().decode()
  assert call(ins=[ptr[0], None, ptr[2], ptr[3]]) != 0 and 'required' in err().decode()
  assert call(outs=[o[0], o[1], None]) != 0 and 'required' in err().decode()
  # a workspace that is missing or short: the targets stay unwritten
  need = lib.sp_nbody_accel_workspace_bytes(f32, 130, 130, 2)
  assert need == 2 * 3 * 130 * 4 and lib.sp_nbody_accel_workspace_bytes(f32, 130, 130, 1) == 0
  ws = be.empty((need,), np.uint8)
  for p, size in ((ws.data_ptr(), need - 1), (None, 0), (None, need)):
    assert call(ws=p, ws_bytes=size) != 0 and 'workspace' in err().decode()
  assert tgt.numpy().tobytes() == marks.tobytes()               # nothing was written
  assert call(ws=ws.data_ptr(), ws_bytes=need) == 0
  assert _same(list(tgt.numpy()), _accel(be, x, y, z, mass, g=1.0, rmin=1.0, splits=2))
  assert call(splits=1) == 0                                    # one range needs no workspace
  assert _same(list(tgt.numpy()), _accel(be, x, y, z, mass, g=1.0, rmin=1.0, splits=1))


# ---- the driver on the device -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('workers', (1, 4))
def test_the_driver_reproduces_the_reference_gpu(workers, dtype):
  ex.check_driver('hip', workers, dtype)


def test_the_expression_form_gpu():
  ex.check_driver('hip', 4, np.float64, 'expr')


def test_one_and_four_workers_agree_bit_for_bit_gpu():
  ex.check_workers_agree('hip')


def test_driver_refusals_gpu():
  ex.check_refusals('hip')
