"""srandom builders (reference spartan/expr/srandom.py): rand / randn / randint.
Values are random by construction (the reference seeds every worker from the clock), so the
tests pin what the reference fixes: shape, tiling, dtype, range and the distribution; on the
GPU additionally that the counter-based generator is a pure function of (seed, position), and -- bit for bit, against
the plain NumPy Philox4x32-10 of tests/philox_ref.py (checked against the published known answers by
tests/test_philox_ref_cpu.py) -- that it is the function include/spartan_hip.h documents."""
import numpy as np
import pytest

import spartan_amd as sp


def _check_builders():
  a = sp.rand(300, 7)
  assert a.shape == (300, 7)
  av = a.glom()
  assert av.dtype == np.float64 and av.min() >= 0.0 and av.max() < 1.0
  assert abs(av.mean() - 0.5) < 0.05
  b = sp.randn(400, 5, tile_hint=(100, 5)).glom()
  assert b.dtype == np.float64 and b.shape == (400, 5)
  assert abs(b.mean()) < 0.15 and abs(b.std() - 1.0) < 0.15
  c = sp.randint(500, 3, low=3, high=9).glom()
  assert c.dtype == np.int64 and c.min() == 3 and c.max() == 8
  # evaluated lazily ONCE per expression (EvalCache): r - r is exactly zero ...
  r = sp.rand(64, 4)
  np.testing.assert_array_equal((r - r).glom(), np.zeros((64, 4)))
  # ... but, as in the reference (checked by running it: its MapMapFusion clones nodes, so the id()-keyed
  # @not_idempotent marker does not reliably survive), the OPTIMISED tree may draw once per occurrence
  r = sp.rand(64, 4)
  e = (r - r).optimized().glom()
  assert e.shape == (64, 4) and np.abs(e).max() < 1.0
  with pytest.raises(AssertionError):
    sp.rand(3, 3, bogus=1)


@pytest.mark.parametrize('workers', [1, 4])
def test_random_builders_host_framework(workers):
  from oracle.np_backend import NumpyBackend
  sp.initialize(backend=NumpyBackend(), num_workers=workers)
  sp.set_random_seed(11)
  try:
    _check_builders()
  finally:
    sp.shutdown()


@pytest.mark.gpu
@pytest.mark.parametrize('workers', [1, 3])
def test_random_builders_hip(workers):
  ctx = sp.initialize('hip', num_workers=workers)
  sp.set_random_seed(11)
  try:
    before = ctx.backend.launches
    _check_builders()
    assert ctx.backend.launches > before
    sp.set_random_seed(11)
    x1 = sp.rand(1000, 9).glom()
    sp.set_random_seed(11)
    x2 = sp.rand(1000, 9).glom()
    np.testing.assert_array_equal(x1, x2)          # same seed, same program -> same bits
    x3 = sp.rand(1000, 9).glom()
    assert not np.array_equal(x1, x3)              # the stream advances
  finally:
    sp.shutdown()


@pytest.mark.gpu
def test_random_fill_kernel_statistics_and_counter_semantics():
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  n = 1 << 20
  for dt, tol in ((np.float32, 2e-3), (np.float64, 2e-3)):
    u = D.empty((n,), dt)
    kernels.random_fill(u, 'uniform', 1234, 0)
    h = u.numpy().astype(np.float64)
    assert h.min() >= 0.0 and h.max() < 1.0
    assert abs(h.mean() - 0.5) < tol and abs(h.var() - 1.0 / 12) < tol
    hist = np.histogram(h, bins=64, range=(0, 1))[0]
    assert np.abs(hist / (n / 64.0) - 1).max() < 0.05
    g = D.empty((n,), dt)
    kernels.random_fill(g, 'normal', 1234, 0)
    gh = g.numpy().astype(np.float64)
    assert abs(gh.mean()) < 5e-3 and abs(gh.var() - 1) < 1e-2
    assert abs(((gh - gh.mean()) ** 4).mean() / gh.var() ** 2 - 3.0) < 0.05       # kurtosis of a normal
    assert abs(np.corrcoef(gh[0::2], gh[1::2])[0, 1]) < 5e-3                       # the Box-Muller pair is uncorrelated
  # position semantics: one fill of n == two consecutive fills of n/2 (launch geometry is irrelevant)
  a = D.empty((n,), np.float64)
  kernels.random_fill(a, 'uniform', 77, 0)
  b = D.empty((n,), np.float64)
  kernels.random_fill(b[: n // 2], 'uniform', 77, 0)
  kernels.random_fill(b[n // 2:], 'uniform', 77, n // 2)
  assert np.array_equal(a.numpy(), b.numpy())
  c = D.empty((n,), np.float64)
  kernels.random_fill(c, 'uniform', 78, 0)
  assert not np.array_equal(a.numpy(), c.numpy())
  k = D.empty((100001,), np.int64)
  kernels.random_fill(k, 'randint', 5, 0, -3, 4)
  kh = k.numpy()
  assert kh.min() == -3 and kh.max() == 3
  assert np.abs(np.bincount(kh + 3, minlength=7) / (len(kh) / 7.0) - 1).max() < 0.05


# ------------------------------------------------------------------------------- sp_random_fill against tests/philox_ref.py
SEEDS = (7, (1 << 40) + 3, 0xfedcba9876543210)            # the second key word is 0, small, and has its top bit set
OFFSETS = (0, 1 << 20, (1 << 33) + 2)                     # the last: pair numbers past 2^32, the second counter word
GRID_STRIDE_N = (1 << 21) + 4097                          # 2^20 + 2049 pairs: more than the 2^20 threads of the capped grid
# [lo, hi): ranges 1, 7, 2^31 and 2^62, negative lo
RANGES = ((-5, -4), (-3, 4), (-2**30, 2**30), (-2**61, 2**61))
ROUND_TO_ONE = ((0, 8628076), (0, 24313416), (2, 16456685), (3, 8975428), (3, 23572345))


def _fill(n, dtype, kind, seed, offset, lo=0, hi=1):
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  out = D.empty((n,), dtype)
  kernels.random_fill(out, kind, seed, offset, lo, hi)
  got = out.numpy()
  assert got.dtype == np.dtype(dtype) and got.shape == (n,)
  return got


def _same_bits(got, want, label):
  assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (label, np.flatnonzero(got != want)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize('seed', SEEDS, ids=hex)
def test_fill_is_philox_bit_for_bit(seed):
  from tests import philox_ref as pr
  n = 1001                                                 # odd: the last pair is half used
  for offset in OFFSETS:
    label = 'seed %#x offset %d' % (seed, offset)
    _same_bits(_fill(n, np.float64, 'uniform', seed, offset), pr.uniform(seed, offset, n), 'uniform ' + label)
    for lo, hi in RANGES:
      _same_bits(_fill(n, np.int64, 'randint', seed, offset, lo, hi), pr.randint(seed, offset, n, lo, hi),
                 'int64 [%d, %d) %s' % (lo, hi, label))
      if -2**31 <= lo and hi <= 2**31:                     # an int32 fill holds a range inside int32
        _same_bits(_fill(n, np.int32, 'randint', seed, offset, lo, hi), pr.randint(seed, offset, n, lo, hi, np.int32),
                   'int32 [%d, %d) %s' % (lo, hi, label))


@pytest.mark.gpu
def test_fill_is_philox_where_the_grid_strides():
  from tests import philox_ref as pr
  n, seed, offset = GRID_STRIDE_N, SEEDS[2], OFFSETS[2]
  _same_bits(_fill(n, np.float64, 'uniform', seed, offset), pr.uniform(seed, offset, n), 'uniform')
  _same_bits(_fill(n, np.int64, 'randint', seed, offset, -2**61, 2**61), pr.randint(seed, offset, n, -2**61, 2**61), 'int64')
  _same_bits(_fill(n, np.int32, 'randint', seed, offset, -3, 4), pr.randint(seed, offset, n, -3, 4, np.int32), 'int32')
  _same_bits(_fill(n, np.float32, 'uniform', seed, offset), pr.uniform(seed, offset, n, np.float32), 'float32 uniform')


@pytest.mark.gpu
def test_split_at_an_odd_cut_made_even():
  """HipBackend.random_tile advances its offset by the tile size made even: 1001 elements at 0, the next fill at
  1002.  Both are windows of the one stream of the seed; element 1001 of the stream is skipped."""
  from tests import philox_ref as pr
  seed = SEEDS[1]
  whole = _fill(2003, np.float64, 'uniform', seed, 0)
  first, second = _fill(1001, np.float64, 'uniform', seed, 0), _fill(1001, np.float64, 'uniform', seed, 1002)
  _same_bits(first, whole[:1001], 'first')
  _same_bits(second, whole[1002:], 'second')
  _same_bits(whole, pr.uniform(seed, 0, 2003), 'whole')


@pytest.mark.gpu
def test_float32_uniform_is_the_cast_kept_below_one():
  """float32(u), except that the u >= 1 - 2^-25 (which round to 1.0) give the largest float32 below 1.  The five
  (seed, position) pairs are such u (tests/test_philox_ref_cpu.py): each is filled as the pair that holds it."""
  from tests import philox_ref as pr
  for seed in SEEDS:
    _same_bits(_fill(4099, np.float32, 'uniform', seed, OFFSETS[1]), pr.uniform(seed, OFFSETS[1], 4099, np.float32),
               'seed %#x' % seed)
  for seed, pos in ROUND_TO_ONE:
    even = pos - (pos & 1)
    got = _fill(2, np.float32, 'uniform', seed, even)
    print('seed %d position %d: %r' % (seed, pos, got[pos - even]))
    assert got[pos - even] < 1, (seed, pos, got)
    _same_bits(got, pr.uniform(seed, even, 2, np.float32), (seed, pos))
    assert got[pos - even] == pr.BELOW_ONE_F32
    assert np.float32(_fill(2, np.float64, 'uniform', seed, even)[pos - even]) == np.float32(1)


@pytest.mark.gpu
def test_normal_within_the_documented_accuracy_of_the_device_functions():
  """Box-Muller on 1 - a and 2 pi b, against tests/philox_ref.py: the same double roundings of 1 - a and of the
  product with 2 pi, then log / sqrt / cos / sin in longdouble.

  Bound for float64, |got - ref| <= K 2^-53 rad with K = philox_ref.NORMAL_K = 36.  The device library documents no
  limits of its own in this tree, so the OpenCL full-profile limits for double stand in: log 3 ulp, sqrt 0 (correctly
  rounded), sin and cos 4.  An ulp is at most 2^-52 of the value = 2 x 2^-53.  One output rad * cos(ang) (or sin)
  carries: log's 3 ulp, halved by the square root but counted whole; sqrt's 0; cos's (or sin's) 4 -- one of the two,
  so max(4, 4); and 1 ulp each for the products -2 * log (exact, counted anyway) and rad * cos (half an ulp).  That is
  3 + 0 + 4 + 2 = 9 ulp <= 18 x 2^-53 of |rad cos| <= rad to first order; K = 4 x 9 doubles it for the second-order
  terms.  The reference's own error (longdouble, 2^-64) is below 2^-10 of the bound.
  Bound for float32 output: the double value rounded once, |got - ref| <= 2^-23 max(rad, 1).
  a == 0 (rad = 0, both elements exactly 0) has probability 2^-53 per pair and cannot be met by a fill; that the map
  gives exactly 0 there is checked on the reference (tests/test_philox_ref_cpu.py)."""
  from tests import philox_ref as pr
  n = (1 << 16) + 1
  for seed, offset in ((SEEDS[0], 0), (SEEDS[2], OFFSETS[2])):
    ref, rad = pr.normal(seed, offset, n)
    got = _fill(n, np.float64, 'normal', seed, offset)
    err = np.asarray(np.abs(got.astype(pr.LD) - ref), np.float64)
    bound = pr.NORMAL_K * 2.0 ** -53 * np.asarray(rad, np.float64)
    print('float64 normal, seed %#x: worst error / bound %.3g' % (seed, float((err / bound).max())))
    assert np.all(err <= bound), (seed, float((err / bound).max()))
    got32 = _fill(n, np.float32, 'normal', seed, offset)
    err32 = np.asarray(np.abs(got32.astype(pr.LD) - ref), np.float64)
    bound32 = 2.0 ** -23 * np.maximum(np.asarray(rad, np.float64), 1)
    print('float32 normal, seed %#x: worst error / bound %.3g' % (seed, float((err32 / bound32).max())))
    assert np.all(err32 <= bound32), (seed, float((err32 / bound32).max()))
    assert np.array_equal(got32, got.astype(np.float32))            # the float32 fill is the float64 one, rounded


@pytest.mark.gpu
def test_an_odd_offset_is_refused_before_any_launch():
  """Elements come in pairs, one Philox block each: a fill that started at an odd position would re-emit the element
  in front of it.  include/spartan_hip.h: an odd offset is an error."""
  import ctypes
  from spartan_amd import _hip
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  out = D.from_numpy(np.full(8, -7.0))
  for kind, lo, hi in (('uniform', 0, 1), ('normal', 0, 1)):
    with pytest.raises(_hip.HipError, match='odd offset'):
      kernels.random_fill(out, kind, 5, 3, lo, hi)
  k = D.from_numpy(np.full(8, -7, np.int64))
  with pytest.raises(_hip.HipError, match='odd offset'):
    kernels.random_fill(k, 'randint', 5, (1 << 33) + 1, -3, 4)
  assert _hip.lib().sp_random_fill(ctypes.c_void_p(out.data_ptr()), _hip.SP_F64, 8, 0, 5, 1, 0, 1, None) != 0
  assert 'odd offset' in _hip.lib().sp_last_error().decode()
  D.synchronize()
  assert np.all(out.numpy() == -7.0) and np.all(k.numpy() == -7)     # nothing was written
