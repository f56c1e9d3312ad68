"""int8, int16, uint16, uint32 and float16 tiles on the GPU, every case against NumPy on the host (the NumPy oracle
backend does not hold these types).  Integer results and float16 results of +, -, *, /, sqrt and casts are bit-exact:
NumPy computes a half operation in float and rounds to half, and so does the kernel (TO_F32 with selector 1 after
every node); exp / log / tanh are within one ulp of half."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import spartan_amd as sp  # noqa: E402
from spartan_amd import _hip, kernels  # noqa: E402
from spartan_amd import devarray as D  # noqa: E402

ALL = [np.dtype(t) for t in (np.float32, np.float64, np.int32, np.int64, np.bool_, np.uint8,
                             np.int8, np.int16, np.uint16, np.uint32, np.float16)]
NEW = ALL[6:]
INTS_NEW = NEW[:4]
F16 = np.dtype(np.float16)
RNG = np.random.RandomState(20160229)
HALVES = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)      # the whole type


def dev(a):
  return D.from_numpy(np.ascontiguousarray(a))


def same(got, want, what=''):
  """Bit for bit; any NaN matches any NaN (the sign / payload of a NaN is not part of NumPy's contract)."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
  if got.dtype.kind == 'f':
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    ok = (np.ascontiguousarray(got).view(u) == np.ascontiguousarray(want).view(u)) | (np.isnan(got) & np.isnan(want))
  else:
    ok = got == want
  if not ok.all():
    i = np.argwhere(~ok)[0]
    raise AssertionError('%s: %d of %d differ, first at %s: got %r want %r' %
                         (what, int((~ok).sum()), ok.size, tuple(i), got[tuple(i)], want[tuple(i)]))


def np_cast(a, dt):
  """ndarray.astype on the host.  float -> uint32 of NaN and of values outside (-2^31, 2^32) is undefined in C, and
  which answer NumPy gives depends on the loop its build picks for the CPU at hand (vectorised or scalar, with or
  without an unsigned conversion instruction).  The reference for that one cast is therefore computed here, as plain
  x86-64 code does it: the int64 truncation (cvttss2si / cvttsd2si on a 64-bit register; INT64_MIN for NaN, +-inf and
  values outside int64), low 32 bits.  Inside (-2^31, 2^32), where every route agrees, NumPy's own astype is asserted
  to give the same."""
  a = np.asarray(a)
  with np.errstate(all='ignore'):
    if np.dtype(dt) == np.uint32 and a.dtype.kind == 'f':
      x = a.astype(np.float64)                      # exact for float16 / float32
      ok = np.isfinite(x) & (x > -2.0 ** 63) & (x < 2.0 ** 63)
      i64 = np.where(ok, np.trunc(np.where(ok, x, 0.0)), 0.0).astype(np.int64)
      i64[~ok] = np.iinfo(np.int64).min
      want = (i64 & 0xFFFFFFFF).astype(np.uint32)
      agreed = ok & (x > -2.0 ** 31) & (x < 2.0 ** 32)
      assert np.array_equal(a.astype(np.uint32)[agreed], want[agreed])
      return want
    return a.astype(dt)


# ---------------------------------------------------------------------------------------------------- casts
@pytest.mark.parametrize('dt', ALL, ids=str)
def test_every_half_casts_to_every_type_and_back(dt):
  d = dev(HALVES)
  want = np_cast(HALVES, dt)
  got = d.astype(dt)
  same(got.numpy(), want, 'float16 -> %s' % dt)
  with np.errstate(all='ignore'):
    same(dev(want).astype(np.float16).numpy(), want.astype(np.float16), '%s -> float16' % dt)


def _half_ties(ft):
  """Exact ties between adjacent halves (subnormal range included), their neighbours in `ft` on both sides (a double
  one step off a tie rounds to the tie as a float: the round trip through float would move it), overflow to inf."""
  bits = np.unique(np.concatenate([np.arange(0, 1200), np.arange(1200, 0x7bff, 61), np.arange(0x7bf0, 0x7bff)]))
  lo = bits.astype(np.uint16).view(np.float16).astype(np.float64)
  hi = (bits + 1).astype(np.uint16).view(np.float16).astype(np.float64)
  mid = ((lo + hi) / 2).astype(ft)        # 12 significant bits: exact in float32 and float64
  vals = np.concatenate([mid, np.nextafter(mid, ft.type(np.inf)), np.nextafter(mid, ft.type(-np.inf)), lo.astype(ft)])
  extra = np.array([0.0, 65504, 65519.996, 65520, 65536, 1e5, np.inf, np.nan, 2.0 ** -25, 2.0 ** -26, 1e-30,
                    np.finfo(ft).tiny, np.finfo(ft).smallest_subnormal, np.finfo(ft).max], ft)
  extra = np.concatenate([extra, np.nextafter(extra[:5], ft.type(0)), np.nextafter(np.array([2.0 ** -25], ft), ft.type(1))])
  vals = np.concatenate([vals, extra])
  return np.concatenate([vals, -vals])


@pytest.mark.parametrize('ft', [np.dtype(np.float32), np.dtype(np.float64)], ids=str)
def test_floats_round_to_half_once(ft):
  x = _half_ties(ft)
  with np.errstate(all='ignore'):
    same(dev(x).astype(np.float16).numpy(), x.astype(np.float16), '%s -> float16' % ft)


def test_int64_to_half_near_the_rounding_steps():
  v = [(2048 + j) * 2 ** k + d for k in range(0, 7) for j in (0, 1, 2, 3) for d in (-1, 0, 1)]
  v += [65503, 65504, 65519, 65520, 65521, 2 ** 24 + 1, 2 ** 40, 2 ** 62]
  x = np.array(v + [-a for a in v], np.int64)
  with np.errstate(all='ignore'):
    same(dev(x).astype(np.float16).numpy(), x.astype(np.float16))


def _edge_grid(dt):
  dt = np.dtype(dt)
  ints = [0, 1, -1, 2, -2, 127, 128, -128, -129, 255, 256, 32767, 32768, -32768, -32769, 65535, 65536, 2 ** 31 - 1,
          2 ** 31, -2 ** 31, -2 ** 31 - 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 63 - 1, -2 ** 63]
  if dt == np.bool_:
    return np.array([False, True])
  if dt.kind in 'iu':
    info = np.iinfo(dt)
    return np.array(sorted({v for v in ints if info.min <= v <= info.max}), dt)
  fl = [float(v) for v in ints] + [0.5, -0.5, 1.5, -1.5, 127.9, -128.9, 255.5, 32767.5, 65535.9, 2147483520.0,
                                   4294967040.0, 1e10, -1e10, 1e19, -1e19, np.inf, -np.inf, np.nan, -0.0]
  with np.errstate(all='ignore'):
    return np.array(fl, np.float64).astype(dt)


@pytest.mark.parametrize('src', ALL, ids=str)
def test_integer_edges_cast_like_numpy(src):
  x = _edge_grid(src)
  d = dev(x)
  targets = NEW if src not in NEW else ALL
  for dst in targets:
    same(d.astype(dst).numpy(), np_cast(x, dst), '%s -> %s' % (src, dst))


# ---------------------------------------------------------------------------------------- per-node narrowing
def _int_pairs(dt):
  """An edge x edge grid of the type, and divisors without 0 (NumPy warns and answers 0; so does the kernel, but -1
  divisors of the minimum are the interesting wrap)."""
  e = _edge_grid(dt)
  a, b = np.meshgrid(e, e, indexing='ij')
  c = np.resize(np.array([v for v in (1, -1, 2, 3, 7, -7, 127, 255, 32767) if np.iinfo(dt).min <= v <= np.iinfo(dt).max], dt), a.shape)
  return np.ascontiguousarray(a), np.ascontiguousarray(b), c


@pytest.mark.parametrize('dt', INTS_NEW, ids=str)
def test_integer_intermediates_wrap_after_every_node(dt):
  a, b, c = _int_pairs(dt)
  A, B, C = dev(a), dev(b), dev(c)
  with np.errstate(all='ignore'):
    same(((A * B) // C).numpy(), (a * b) // c, '(a * b) // c')
    same(((A - B) % C).numpy(), (a - b) % c, '(a - b) % c')
    same((A + 1).numpy(), a + 1, 'a + 1')
  assert (A + 1).dtype == dt


def _half_grid():
  e = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 1.5, 3.0, 0.1, 0.333, 1 / 3.0, 2.0 ** -14, 2.0 ** -15, 2.0 ** -24, 3 * 2.0 ** -24,
                1023 * 2.0 ** -24, 2047.0, 2048.0, 2049.0, 4095.0, 255.9, 256.1, 1000.5, 60000.0, 65504.0, 32768.0, 181.0,
                181.125, 0.007, 1.0009765625, 0.99951171875, np.inf, np.nan], np.float16)
  e = np.concatenate([e, -e[2:]])             # 62 values
  a, b = np.meshgrid(e, e, indexing='ij')
  c = np.resize(e[::-1], a.shape)
  return np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c)


def test_half_intermediates_round_after_every_node():
  a, b, c = _half_grid()
  A, B, C = dev(a), dev(b), dev(c)
  with np.errstate(all='ignore'):
    same((A * B + C).numpy(), a * b + c, 'a * b + c')
    same((A / B).numpy(), a / b, 'a / b')
    same((A - B).numpy(), a - b, 'a - b')
    same(np.sqrt(A).numpy(), np.sqrt(a), 'sqrt(a)')
    same((A * 1.5).numpy(), a * 1.5, 'a * 1.5 (weak scalar keeps float16)')


@pytest.mark.parametrize('fn', [np.exp, np.log, np.tanh], ids=lambda f: f.__name__)
def test_half_transcendentals_within_one_ulp(fn):
  x = HALVES[np.isfinite(HALVES)]
  with np.errstate(all='ignore'):
    got = fn(dev(x)).numpy()
    ref = fn(x.astype(np.float64))
    want = ref.astype(np.float16)
  assert got.dtype == F16
  # one ulp of half AT the reference value: the neighbours of the correctly rounded half
  lo, hi = np.nextafter(want, F16.type(-np.inf)), np.nextafter(want, F16.type(np.inf))
  ok = (got == want) | (got == lo) | (got == hi) | (np.isnan(got) & np.isnan(want))
  assert ok.all(), (int((~ok).sum()), x[~ok][:5], got[~ok][:5], want[~ok][:5])


# ------------------------------------------------------------------------------------------------- shapes
def _values(dt, shape):
  dt = np.dtype(dt)
  if dt.kind == 'f':
    return (RNG.randint(-4096, 4096, size=shape) / 64.0).astype(dt)
  info = np.iinfo(dt)
  return RNG.randint(max(info.min, -2 ** 31), min(info.max, 2 ** 31 - 1) + 1, size=shape).astype(dt)


@pytest.mark.parametrize('dt', [np.dtype(np.int8), np.dtype(np.uint16), F16], ids=str)
def test_shapes_reach_every_path(dt):
  def check(x, y, what):
    with np.errstate(all='ignore'):
      want = x * y + x
    xd = x if isinstance(x, D.DevArray) else dev(x)
    yd = y if isinstance(y, D.DevArray) else dev(y)
    got = (xd * yd + xd).numpy()
    # (a DevArray's result of 0-d operands is one element of shape (1,), for every dtype: the value is what is checked)
    same(got.reshape(want.shape) if want.shape == () else got, want, what)
  for shape in [(7,), (), (5, 3001), (64, 4096)]:
    check(_values(dt, shape), _values(dt, shape), str(shape))
  big, other = _values(dt, (64, 4096)), _values(dt, (64, 4095))
  bd = dev(big)
  with np.errstate(all='ignore'):
    same((bd[:, 1:] * dev(other) + bd[:, 1:]).numpy(), big[:, 1:] * other + big[:, 1:], 'sliced [:, 1:]')
  check(_values(dt, (3, 1, 5)), _values(dt, (1, 4, 1)), 'broadcast (3,1,5) o (1,4,1)')
  check(big, _values(dt, (4096,)), 'row vector down (64, 4096)')


# --------------------------------------------------------------------------------------------- reductions
def _count_nonzero(x, axis):
  """The builder's rule (the reference's sorting.py:126-133): np.count_nonzero for axis=None, (x > 0).sum(axis) along an
  axis -- the number of POSITIVE elements."""
  return np.asarray(np.count_nonzero(x) if axis is None else (x > 0).sum(axis=axis))


@pytest.fixture
def one_worker():
  sp.initialize('hip', num_workers=1)
  yield sp
  sp.shutdown()


@pytest.mark.parametrize('shape', [(5, 3001), (64, 4096)], ids=str)
@pytest.mark.parametrize('dt', INTS_NEW, ids=str)
def test_integer_reductions(one_worker, dt, shape):
  x = _values(dt, shape)
  x[x == 0] = 1
  x.ravel()[::977] = 0
  small = np.where(RNG.rand(*shape) < 0.01, 2, 1).astype(dt)      # products that wrap only mod 2^64
  X, S = sp.from_numpy(x), sp.from_numpy(small)
  for axis in (None, 0, 1):
    for name, npf, arr, src in (('sum', np.sum, X, x), ('prod', np.prod, S, small), ('max', np.max, X, x),
                                ('min', np.min, X, x), ('all', np.all, X, x), ('any', np.any, X, x),
                                ('count_nonzero', None, X, x)):
      got = np.asarray(getattr(sp, name)(arr, axis).glom())
      with np.errstate(all='ignore'):
        if name == 'count_nonzero':
          want = _count_nonzero(src, axis)
        elif name in ('sum', 'prod'):
          want = np.asarray(npf(src.astype(np.int64), axis=axis))      # exact in int64 ...
        else:
          want = np.asarray(npf(src, axis=axis))
      # ... and the builders' dtype_fn names the result type (sum / prod / max / min: the operand's own, so sums wrap
      # at its width; all / any: bool; count_nonzero: int64); the value wraps into it like astype
      rule = {'all': np.dtype(np.bool_), 'any': np.dtype(np.bool_), 'count_nonzero': np.dtype(np.int64)}.get(name, dt)
      assert got.dtype == rule, (name, axis, got.dtype, rule)
      assert np.array_equal(got, want.astype(rule)), (name, axis)


@pytest.mark.parametrize('shape', [(5, 3001), (64, 4096)], ids=str)
def test_half_reductions(one_worker, shape):
  x = (RNG.randint(-512, 513, size=shape) / 256.0).astype(np.float16)          # |x| <= 2, |S| far below 65504
  X = sp.from_numpy(x)
  x64 = x.astype(np.float64)
  for axis in (None, 0, 1):
    got = np.asarray(sp.sum(X, axis).glom())
    assert got.dtype == F16
    S, A = x64.sum(axis=axis), np.abs(x64).sum(axis=axis)
    assert (np.abs(S) < 65504).all()
    bound = 2.0 ** -11 * np.abs(S) + 1e-6 * A          # one rounding to half + the fp32 accumulation bound
    err = np.abs(got.astype(np.float64) - S)
    assert (err <= bound).all(), (axis, float(err.max()), float(bound.min()))
    same(np.asarray(sp.max(X, axis).glom()), np.asarray(x.max(axis=axis)), 'max')
    same(np.asarray(sp.min(X, axis).glom()), np.asarray(x.min(axis=axis)), 'min')
    same(np.asarray(sp.any(X, axis).glom()), np.asarray(x.any(axis=axis)), 'any')
    same(np.asarray(sp.all(X, axis).glom()), np.asarray(x.all(axis=axis)), 'all')
    same(np.asarray(sp.count_nonzero(X, axis).glom()), _count_nonzero(x, axis).astype(np.int64), 'count_nonzero')
  # products of powers of two are exact in any order and any precision
  p = np.where(RNG.rand(*shape) < 0.002, 2.0, 1.0).astype(np.float16)
  p.ravel()[::7919] = 0.5
  for axis in (None, 0, 1):
    same(np.asarray(sp.prod(sp.from_numpy(p), axis).glom()), np.asarray(p.astype(np.float64).prod(axis=axis).astype(np.float16)), 'prod')


@pytest.mark.parametrize('dt', [np.dtype(np.int8), np.dtype(np.uint16), F16], ids=str)
def test_arg_reductions_with_duplicates_and_nan(dt):
  x = _values(dt, (5, 3001))
  top = np.iinfo(dt).max if dt.kind != 'f' else dt.type(1000)
  bot = np.iinfo(dt).min if dt.kind != 'f' else dt.type(-1000)
  x[:, 17] = top; x[:, 2900] = top; x[2, :] = np.where(np.arange(3001) % 2, x[2, :], top)
  x[:, 40] = bot; x[:, 41] = bot
  d = dev(x)
  for axis in (None, 0, 1):
    assert np.array_equal(d.argmax(axis).numpy(), np.argmax(x, axis=axis)), ('argmax', axis)
    assert np.array_equal(d.argmin(axis).numpy(), np.argmin(x, axis=axis)), ('argmin', axis)


def test_half_argmax_nan_gives_the_sentinel(one_worker):
  x = _values(F16, (5, 3001))
  x[3, 77] = np.nan
  got = np.asarray(sp.argmax(sp.from_numpy(x), 1).glom())
  want = np.argmax(np.where(np.isnan(x), -np.inf, x), axis=1)
  want[3] = x.size                     # the reference's `a == b` never matches NaN: the sentinel prod(shape)
  assert np.array_equal(got, want), (got, want)


# -------------------------------------------------------------------------------------------------- merge
def _merge_values(dt, shape, seed):
  rng = np.random.RandomState(seed)
  dt = np.dtype(dt)
  if dt == np.bool_:
    return rng.rand(*shape) < 0.5
  if dt.kind == 'f':
    v = rng.choice(np.array([0, 1, -1, 0.5, 2, 127, 0.99, 100.25, 3.0, -7.5, 255, 1000.5], np.float64), size=shape)
    return v.astype(dt)
  info = np.iinfo(dt)
  edges = np.array(sorted({max(info.min, min(info.max, e)) for e in (0, 1, -1, 2, 3, 127, -128, 255, 32767, -32768, 65535,
                                                                    info.min, info.max)}), np.float64)
  return rng.choice(edges, size=shape).astype(dt)


@pytest.mark.parametrize('tile_dt', ALL, ids=str)
def test_merge_every_pair_reducer_and_mask_mode(tile_dt):
  reducers = {'NONE': None, 'ADD': np.add, 'MUL': np.multiply, 'MAX': np.maximum, 'MIN': np.minimum,
              'AND': np.logical_and, 'OR': np.logical_or}
  for upd_dt in ALL:
    old = _merge_values(tile_dt, (9, 11), 1)
    mask = np.random.RandomState(3).rand(9, 11) < 0.5
    for (ul, lr) in (((1, 2), (7, 10)), ((3, 4), (8, 11))):               # a (6, 8) box and a (5, 7) box
      box = tuple(slice(a, b) for a, b in zip(ul, lr))
      upd = _merge_values(upd_dt, tuple(b - a for a, b in zip(ul, lr)), 2)
      names = ['NONE', 'ADD', 'MUL', 'MAX', 'MIN'] + (['AND', 'OR'] if tile_dt == np.bool_ else [])
      for name in names:
        for mode in (_hip.MASK_ALL_CLEAR, _hip.MASK_ALL_SET, _hip.MASK_ARRAY):
          t, m = dev(old), dev(mask.astype(np.uint8))
          kernels.update(t, ul, lr, dev(upd), name, mode, m if mode == _hip.MASK_ARRAY else None)
          was_set = {_hip.MASK_ALL_CLEAR: np.zeros_like(mask[box]), _hip.MASK_ALL_SET: np.ones_like(mask[box]),
                     _hip.MASK_ARRAY: mask[box]}[mode]
          with np.errstate(all='ignore'):
            merged = upd if name == 'NONE' else reducers[name](old[box], upd)
            want = old.copy()
            want[box] = np.where(was_set, np_cast(np.asarray(merged), tile_dt), np_cast(upd, tile_dt))
          same(t.numpy(), want, '%s tile, %s update, %s, mask mode %d, box %s' % (tile_dt, upd_dt, name, mode, (ul, lr)))


# ------------------------------------------------------------------------------------------------- copies
@pytest.mark.parametrize('dt', [np.dtype(np.int16), np.dtype(np.uint16), F16], ids=str)
def test_copies_of_two_byte_tiles(dt):
  src = _values(dt, (37, 53))
  s = dev(src)
  dst = D.from_numpy(np.zeros((41, 59), dt))
  kernels.slice_copy(dst, 3 * 59 + 5, (59, 1), s, 1 * 53 + 3, (53, 1), (21, 33))       # odd offsets, odd extents
  want = np.zeros((41, 59), dt)
  want[3:24, 5:38] = src[1:22, 3:36]
  same(dst.numpy(), want, 'box copy')
  same(s.t().contiguous().numpy(), np.ascontiguousarray(src.T), 'transpose')
  same(s[1:, 3:].t().contiguous().numpy(), np.ascontiguousarray(src[1:, 3:].T), 'transpose of a slice')
  idx = np.array([5, 0, -1, 36, 5, 17], np.int64)
  same(kernels.gather_rows(s, dev(idx)).numpy(), src[idx], 'gather rows (106-byte rows)')
  even = _values(dt, (19, 64))
  same(kernels.gather_rows(dev(even), dev(idx[:4] % 19)).numpy(), even[idx[:4] % 19], 'gather rows (128-byte rows)')


# --------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize('workers', [1, 3])
def test_end_to_end(workers, tmp_path):
  a = RNG.randint(-128, 128, size=(96, 130)).astype(np.int8)
  b = RNG.randint(0, 256, size=(96, 130)).astype(np.uint8)
  sp.initialize('hip', num_workers=workers)
  try:
    e = sp.from_numpy(a) * 3 + sp.from_numpy(b)
    want = a * 3 + b
    assert want.dtype == np.int16
    same(np.asarray(e.glom()), want, 'int8 * 3 + uint8')
    s = sp.sum(e, axis=0)
    got = np.asarray(s.glom())
    assert got.dtype == np.int16                       # sum's dtype_fn: the operand's own type, wrapped at its width
    assert np.array_equal(got, want.sum(axis=0).astype(np.int16))
    h = sp.astype(e, np.float16)
    same(np.asarray(h.glom()), want.astype(np.float16), 'astype(float16)')
    with np.errstate(all='ignore'):
      same(np.asarray(sp.sqrt(h).glom()), np.sqrt(want.astype(np.float16)), 'sqrt of float16')
    x = (RNG.randint(-2000, 2000, size=(50, 37)) / 16.0).astype(np.float16)
    path = str(tmp_path / 'half')
    sp.save(sp.from_numpy(x), 'x', path, False)
    same(np.asarray(sp.load('x', path, False).glom()), x, 'save / load of float16')
  finally:
    sp.shutdown()


# -------------------------------------------------------------------------------------------------- tiers
_TIER_CHILD = r'''
import numpy as np, sys
from spartan_amd import _hip
from spartan_amd import devarray as D
lib = _hip.lib()
rng = np.random.RandomState(5)
a8, b8 = rng.randint(-128, 128, size=(2, 257, 64)).astype(np.int8)
ah, bh = (rng.randint(-4096, 4096, size=(2, 257, 64)) / 32.0).astype(np.float16)
def run():
  A, B, H, G = D.from_numpy(a8), D.from_numpy(b8), D.from_numpy(ah), D.from_numpy(bh)
  return ((A * B - A) * B).numpy(), ((H * G - H) / G + H).numpy()
lib.sp_jit_configure(0, -1)
want = run()
if lib.sp_jit_configure(1, 1) != 1:
  print('NOJIT'); sys.exit(0)     # the parent fails on this: the tier is part of the build
before = lib.sp_jit_compiled_count()
got = run()
lib.sp_jit_wait()
after = lib.sp_jit_compiled_count()
ok = all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))
with np.errstate(all='ignore'):
  ref = ((a8 * b8 - a8) * b8, (ah * bh - ah) / bh + ah)
okref = all(np.array_equal(g, r, equal_nan=True) and g.dtype == r.dtype for g, r in zip(got, ref))
print('RESULT', ok, okref, before, after)
'''


def test_specialised_tier_is_bit_identical_to_the_interpreter():
  """A fresh child process (never a re-exec of one that holds the GPU) with synchronous run-time specialisation from
  one element up: the int8 and the float16 program give the interpreter's bits, and kernels were compiled."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  env = dict(os.environ, SP_JIT_SYNC='1', SP_JIT_MIN_ELEMS='1', SPARTAN_JIT_CACHE='off')
  p = subprocess.run([sys.executable, '-c', _TIER_CHILD], env=env, cwd=root, capture_output=True, text=True, timeout=300)
  assert p.returncode == 0, p.stderr[-2000:]
  line = p.stdout.strip().splitlines()[-1]
  assert line != 'NOJIT', 'run-time specialisation is not usable (libhiprtc did not load)'
  tag, ok, okref, before, after = line.split()
  assert tag == 'RESULT' and ok == 'True' and okref == 'True', line
  assert int(after) > int(before), line


# ------------------------------------------------------------------------------------- out-of-scope kernels
@pytest.mark.parametrize('dt', [np.dtype(np.int8), F16], ids=str)
def test_kernels_outside_the_tile_path_refuse(one_worker, dt):
  x = sp.from_numpy(_values(dt, (16, 16)))
  for what, build in (('dot', lambda: sp.dot(x, x)), ('sort', lambda: sp.sort(x, 1)), ('scan', lambda: sp.scan(x, axis=0))):
    with pytest.raises(Exception, match='dtype %s is not supported by .* of the HIP tile backend' % dt):
      build().glom()
