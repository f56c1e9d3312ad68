"""Data movement on the device against NumPy, byte for byte: the sp_slice_copy and sp_update tables of
tests/copy_cases.py, DevArray views read and written through the copy kernels, overlapping assignments,
sp_stream_copy_wg, sp_memset and the blob box transfers through ctypes.  There is no tolerance anywhere: these
operations move values (the merge applies the one IEEE operation NumPy applies; the one cell IEEE 754 leaves open,
the payload of NaN + NaN, is the update's, as copy_cases.nan_pinned_add spells out)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from spartan_amd import _hip, kernels  # noqa: E402
from spartan_amd import devarray as D  # noqa: E402
from tests import copy_cases as cc  # noqa: E402
from tests.test_devarray import _random_index  # noqa: E402


def dev_words(a):
  """A 1-d array of unsigned words on the device (uint64 travels as int64: the bytes are what counts)."""
  return D.from_numpy(a.view(cc.DEVICE_DTYPE[a.dtype.itemsize]) if a.dtype.kind == 'u' else a)


def same(got, want, what):
  cc.assert_same_bytes(np.ascontiguousarray(got), np.ascontiguousarray(want), None, what)


# ------------------------------------------------------------------------------------------------- sp_slice_copy
_COPY_GROUPS = ['es1', 'es2', 'es4', 'es8'] + [c.name for c in cc.COPY_CASES if c.big]


@pytest.mark.parametrize('group', _COPY_GROUPS)
def test_slice_copy_table(group):
  rows = [c for c in cc.COPY_CASES if (c.name == group if c.big else (not c.big and group == 'es%d' % c.es))]
  assert rows
  failures = []
  for i, case in enumerate(rows):
    dst, src = cc.copy_inputs(case, seed=i)
    want, inside = cc.copy_expected(case, dst, src)
    dd, ds = dev_words(dst), dev_words(src)
    assert dd.data_ptr() % 16 == 0 and ds.data_ptr() % 16 == 0
    # the row reaches the kernel it names with the REAL pointers as well
    assert cc.copy_path_of(case, dd.data_ptr(), ds.data_ptr()) == cc.copy_path_expected(case), case.name
    kernels.slice_copy(dd, case.dst_origin, case.dst_strides, ds, case.src_origin, case.src_strides, case.shape)
    msg = cc.first_difference(dd.numpy().view(dst.dtype), want, inside, case.name)
    if msg is None:
      msg = cc.first_difference(ds.numpy().view(src.dtype), src, None, case.name + ' (the SOURCE changed)')
    if msg is not None:
      failures.append(msg)
  assert not failures, '%d of %d rows:\n%s' % (len(failures), len(rows), '\n'.join(failures[:20]))


# ------------------------------------------------------------------------------------------------- sp_update
def _update_group(c):
  if c.big:
    return c.name
  if 'eligible' in c.name or 'break' in c.name:
    return 'widths %s' % c.cls
  return 'rank %d' % len(c.tile_shape)


_UPDATE_GROUPS = sorted({_update_group(c) for c in cc.UPDATE_CASES})


@pytest.mark.parametrize('group', _UPDATE_GROUPS)
def test_update_table(group):
  rows = [c for c in cc.UPDATE_CASES if _update_group(c) == group]
  failures = []
  for i, case in enumerate(rows):
    tb, mb, ub = cc.update_inputs(case, seed=i)
    want_t, want_m, in_t, in_m = cc.update_expected(case, tb, mb, ub)
    dt, dm, du = D.from_numpy(tb), D.from_numpy(mb), D.from_numpy(ub)
    assert dt.data_ptr() % 16 == 0 and du.data_ptr() % 16 == 0
    assert cc.update_path_of(case, dt.data_ptr(), du.data_ptr()) == (case.cls, case.vec), case.name
    tile, mask, upd = cc.update_views(case, dt, dm, du)
    kernels.update(tile, case.ul, case.lr, upd, case.reducer, case.mask_mode, mask if case.with_mask else None)
    msg = (cc.first_difference(dt.numpy(), want_t, in_t, case.name + ' [tile]') or
           cc.first_difference(dm.numpy(), want_m, in_m, case.name + ' [mask]') or
           cc.first_difference(du.numpy(), ub, None, case.name + ' [the UPDATE changed]'))
    if msg is not None:
      failures.append(msg)
  assert not failures, '%d of %d rows:\n%s' % (len(failures), len(rows), '\n'.join(failures[:20]))


# ------------------------------------------------------------------------------------------------- views on the device
_FUZZ_DTYPES = [np.uint8, np.int16, np.float32, np.float64, np.float16, np.int64, np.int8, np.int32]
_EXTENTS = (1, 2, 3, 16, 17, 64, 65)


def _fuzz_shape(rng, nd, cap=1 << 20):
  shape = [int(rng.choice(_EXTENTS)) for _ in range(nd)]
  while int(np.prod(shape, dtype=np.int64)) > cap:
    k = int(np.argmax(shape))
    shape[k] = int(rng.choice([e for e in _EXTENTS if e < shape[k]]))
  return tuple(shape)


def _random_values(dt, shape, seed):
  dt = np.dtype(dt)
  n = int(np.prod(shape, dtype=np.int64))
  return cc.random_bytes(n * dt.itemsize, seed).view(dt).reshape(shape)


def _random_view(rng, a, d, steps=3):
  """The same chain of basic indices, permutations and axis moves applied to the NumPy array and the device array."""
  for _ in range(steps):
    op = rng.randint(0, 3)
    if op == 0 or a.ndim < 2:
      idx = _random_index(rng, a.shape)
      # (all integers: NumPy would hand back a scalar, not the 0-d view the device array gives)
      a, d = a[idx if Ellipsis in idx else idx + (Ellipsis,)], d[idx]
    elif op == 1:
      perm = tuple(int(p) for p in rng.permutation(a.ndim))
      a, d = a.transpose(perm), d.permute(*perm)
    else:
      s, t = int(rng.randint(0, a.ndim)), int(rng.randint(0, a.ndim))
      a, d = np.moveaxis(a, s, t), d.movedim(s, t)
    assert d.shape == a.shape
  return a, d


@pytest.mark.parametrize('part', range(4))
def test_views_read_on_the_device_match_numpy(part):
  rng = np.random.RandomState(100 + part)
  for case in range(40):
    dt = np.dtype(_FUZZ_DTYPES[(case + 2 * part) % len(_FUZZ_DTYPES)])
    shape = _fuzz_shape(rng, rng.randint(1, 5))
    base = _random_values(dt, shape, 10 * case + part)
    dbase = D.from_numpy(base)
    a, d = _random_view(rng, base, dbase)
    what = 'case %d.%d: %s %s -> shape %s strides %s' % (part, case, dt, shape, d.shape, d.strides)
    same(d.numpy(), a, what + ' numpy()')
    c = d.copy()
    assert c.shape == a.shape and (c.is_contiguous() or a.size == 0) and c.storage is not d.storage, what
    same(c.numpy(), a, what + ' copy()')
    same(d.contiguous().numpy(), a, what + ' contiguous()')
    same(dbase.numpy(), base, what + ' (reading changed the base)')


@pytest.mark.parametrize('part', range(4))
def test_views_written_on_the_device_match_numpy(part):
  """d[idx] = values (a host array and a device array) and d[idx].fill(c): the WHOLE base buffer against NumPy's."""
  rng = np.random.RandomState(200 + part)
  for case in range(30):
    dt = np.dtype(_FUZZ_DTYPES[(case + 2 * part + 1) % len(_FUZZ_DTYPES)])
    shape = _fuzz_shape(rng, rng.randint(1, 5))
    base = _random_values(dt, shape, 10 * case + part + 5)
    state = rng.get_state()
    for mode in ('host values', 'device values', 'fill'):
      rng.set_state(state)                # (the three modes of a case write through the same view)
      ref = base.copy()
      dbase = D.from_numpy(base)
      a, d = _random_view(rng, ref, dbase, steps=2)
      what = 'case %d.%d %s: %s %s -> shape %s strides %s' % (part, case, mode, dt, shape, d.shape, d.strides)
      if mode == 'fill':
        c = dt.type(1.5) if dt.kind == 'f' else dt.type(7)
        a[...] = c
        d.fill(c)
      else:
        values = _random_values(dt, a.shape, 7 * case + 3)
        a[...] = values
        d[...] = values if mode == 'host values' else D.from_numpy(values)
      same(dbase.numpy(), ref, what)


def test_views_of_five_and_six_dimensions():
  """More than SP_MAX_DIMS axes: paste launches the copy kernel once per index of the leading axes."""
  rng = np.random.RandomState(31)
  for shape, dt in (((3, 4, 2, 5, 3, 4), np.float32), ((2, 3, 4, 5, 6), np.int64), ((4, 3, 2, 3, 2, 5), np.uint8),
                    ((2, 17, 3, 2, 16), np.int16)):
    base = _random_values(dt, shape, len(shape))
    nd = len(shape)
    for trial in range(6):
      perm = tuple(int(p) for p in rng.permutation(nd))
      idx = tuple(slice(None) if rng.randint(0, 2) else slice(int(rng.randint(0, 2)), None, int(rng.choice([1, 2, -1])))
                  for _ in range(nd))
      ref = base.copy()
      dbase = D.from_numpy(base)
      a, d = ref.transpose(perm)[idx], dbase.permute(*perm)[idx]
      assert a.ndim == nd and d.shape == a.shape and a.size
      what = '%s %s perm %s idx %s' % (np.dtype(dt), shape, perm, idx)
      same(d.numpy(), a, what + ' numpy()')
      same(d.copy().numpy(), a, what + ' copy()')
      values = _random_values(dt, a.shape, trial)
      a[...] = values
      d[...] = D.from_numpy(values) if trial % 2 else values
      same(dbase.numpy(), ref, what + ' assignment')


# ------------------------------------------------------------------------------------------------- overlap
@pytest.mark.parametrize('name', ['shift up', 'shift columns left', 'reverse', 'transpose in place', 'shift rows of a view'])
def test_overlapping_assignment_equals_numpy(name):
  """NumPy copies the source first when it overlaps the destination; so must a DevArray assignment."""
  if name == 'shift up':
    a = _random_values(np.float32, (1 << 20,), 1)
    act = lambda x: x.__setitem__(slice(1, None), x[:-1])          # noqa: E731
  elif name == 'shift columns left':
    a = _random_values(np.float32, (1024, 1024), 2)
    act = lambda x: x.__setitem__((slice(None), slice(None, -1)), x[:, 1:])          # noqa: E731
  elif name == 'reverse':
    a = _random_values(np.int64, (1 << 20,), 3)
    act = lambda x: x.__setitem__(slice(None), x[::-1])          # noqa: E731
  elif name == 'transpose in place':
    a = _random_values(np.float32, (1024, 1024), 4)
    act = lambda x: x.__setitem__(slice(None), x.T if isinstance(x, np.ndarray) else x.t())          # noqa: E731
  else:
    a = _random_values(np.uint8, (1100, 1000), 5)
    act = lambda x: x[50:, 3:].__setitem__(slice(1, None), x[50:, 3:][:-1])          # noqa: E731
  d = D.from_numpy(a)
  ref = a.copy()
  act(ref)
  act(d)
  same(d.numpy(), ref, name)
  assert ref.tobytes() != a.tobytes()


# ------------------------------------------------------------------------------------------------- sp_stream_copy_wg
MiB = 1 << 20
_G = 64                                   # guard bytes on both sides (a multiple of 16)
_SMALL = (0, 1, 15, 16, 17, 4095, 4096 + 16 + 5, MiB + 3)
_LARGE = (32 * MiB - 16, 32 * MiB, 32 * MiB + 16 + 7)
_OFFSETS = [(o, o) for o in (0, 1, 4, 8, 16)] + [(0, 1), (1, 0), (4, 8), (16, 4), (8, 16), (0, 16), (16, 1)]


@pytest.fixture(scope='module')
def stream_buffers():
  """One source of random bytes and one destination, both a little over 32 MiB, and the destination's pattern."""
  n = _LARGE[-1] + 2 * _G + 16
  src = cc.random_bytes(n, 77)
  pattern = cc.pattern_words(1, n)
  return src, D.from_numpy(src), pattern, D.empty((n,), np.uint8)


def _stream_copy_case(bufs, nbytes, doff, soff, wg, stream=None):
  src, dsrc, pattern, ddst = bufs
  span = nbytes + 2 * _G + 16             # what of the destination is reset and read back
  assert ddst.data_ptr() % 16 == 0 and dsrc.data_ptr() % 16 == 0 and span <= ddst.numel()
  ddst[:span].upload(pattern[:span])
  want = pattern[:span].copy()
  want[_G + doff:_G + doff + nbytes] = src[_G + soff:_G + soff + nbytes]
  if stream is None:
    kernels.stream_copy(ddst[_G + doff:], dsrc[_G + soff:], nbytes, wg)
  else:
    uploaded, copied = D.Event(), D.Event()
    stream.wait_event(uploaded.record())                       # behind the upload on the launch stream
    kernels.stream_copy(ddst[_G + doff:], dsrc[_G + soff:], nbytes, wg, stream=stream)
    D.current_stream().wait_event(copied.record(stream))       # and the read-back behind the copy
    copied.synchronize()
  inside = np.zeros(span, bool)
  inside[_G + doff:_G + doff + nbytes] = True
  return cc.first_difference(ddst[:span].numpy(), want, inside,
                             'stream_copy of %d bytes, dst +%d, src +%d, max_workgroups %d' % (nbytes, doff, soff, wg))


@pytest.mark.parametrize('nbytes', _SMALL)
def test_stream_copy_small(stream_buffers, nbytes):
  failures = [m for doff, soff in _OFFSETS for wg in (0, 1, 3, 1 << 20)
              for m in [_stream_copy_case(stream_buffers, nbytes, doff, soff, wg)] if m]
  assert not failures, '\n'.join(failures[:10])


@pytest.mark.parametrize('nbytes', _LARGE)
def test_stream_copy_large(stream_buffers, nbytes):
  """Around the 32 MiB threshold of the non-temporal kernel (it needs both pointers aligned and at least 32 MiB of
  whole 16-byte words): aligned, aligned on a bounded grid, unaligned (the byte kernel end to end), mixed."""
  combos = [(0, 0, 0), (16, 16, 3), (0, 16, 1), (16, 0, 1 << 20), (1, 1, 0), (4, 8, 3), (8, 8, 1 << 20)]
  failures = [m for doff, soff, wg in combos for m in [_stream_copy_case(stream_buffers, nbytes, doff, soff, wg)] if m]
  assert not failures, '\n'.join(failures[:10])


def test_stream_copy_on_a_side_stream_and_whole_arrays(stream_buffers):
  side = D.Stream()
  for nbytes, doff, soff, wg in ((MiB + 3, 0, 0, 0), (4096 + 16 + 5, 1, 4, 3), (32 * MiB, 16, 0, 0)):
    msg = _stream_copy_case(stream_buffers, nbytes, doff, soff, wg, stream=side)
    assert msg is None, msg
  side.synchronize()
  # nbytes left out: all of the source; sp_stream_copy is the same entry point with the full grid
  a = cc.random_bytes(100003, 5)
  out = D.from_numpy(cc.pattern_words(1, 100003 + 16))
  kernels.stream_copy(out, D.from_numpy(a))
  same(out.numpy(), np.concatenate([a, cc.pattern_words(1, 100003 + 16)[100003:]]), 'stream_copy of a whole array')
  f = _random_values(np.float64, (4099,), 9)
  out = D.from_numpy(np.zeros(4099, np.float64))
  _hip.check(_hip.lib().sp_stream_copy(C.c_void_p(out.data_ptr()), C.c_void_p(D.from_numpy(f).data_ptr()), f.nbytes,
                                       D.current_stream().ptr))
  same(out.numpy(), f, 'sp_stream_copy')


# ------------------------------------------------------------------------------------------------- sp_memset, zeros
def test_memset_and_zeros():
  n = MiB + 5 + 2 * _G + 16
  pattern = cc.pattern_words(1, n)
  buf = D.empty((n,), np.uint8)
  failures = []
  for value in (0, 0x5A, 0xFF):
    for nbytes in (0, 1, 3, 17, 4097, MiB + 5):
      for off in (0, 1, 3, 16):
        span = _G + off + nbytes + _G
        buf[:span].upload(pattern[:span])
        _hip.check(_hip.lib().sp_memset(C.c_void_p(buf.data_ptr() + _G + off), value, nbytes, D.current_stream().ptr))
        want = pattern[:span].copy()
        want[_G + off:_G + off + nbytes] = value
        inside = np.zeros(span, bool)
        inside[_G + off:_G + off + nbytes] = True
        msg = cc.first_difference(buf[:span].numpy(), want, inside, 'memset 0x%02x, %d bytes at +%d' % (value, nbytes, off))
        if msg:
          failures.append(msg)
  assert not failures, '\n'.join(failures[:10])
  with pytest.raises(_hip.HipError):
    _hip.check(_hip.lib().sp_memset(None, 0, 16, D.current_stream().ptr))
  # zeros() of memory the pool hands out again: every byte is zero, whatever was there
  for shape, dt in (((7,), np.uint8), ((3, 5), np.float32), ((1025, 3), np.float64), ((), np.int64), ((0, 4), np.int32),
                    ((129, 65), np.int16), ((4099,), np.bool_)):
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
    dirty = D.from_numpy(np.full(max(nbytes, 1), 0xA5, np.uint8))
    del dirty                                       # (back to the pool: the next array of this size class gets it)
    z = D.zeros(shape, dt)
    assert z.shape == tuple(shape) and z.dtype == np.dtype(dt)
    same(z.numpy(), np.zeros(shape, dt), 'zeros(%s, %s)' % (shape, np.dtype(dt)))


# ------------------------------------------------------------------------------------------------- blobs through ctypes
_BLOB_DTYPES = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.float64}
_NULL = C.c_void_p(0)


class Blob(object):
  """A blob of the tile store driven through the C-ABI alone."""

  def __init__(self, shape, dtype):
    self.shape, self.dtype = tuple(shape), np.dtype(dtype)
    self.h = C.c_uint64()
    _hip.check(_hip.lib().sp_blob_create(_hip.i64_array(self.shape), len(self.shape), _hip.sp_dtype(self.dtype), C.byref(self.h)))

  def close(self):
    if self.h is not None:
      _hip.check(_hip.lib().sp_blob_destroy(self.h))
      self.h = None

  __del__ = close

  @staticmethod
  def _box(ul, lr):
    return (None if ul is None else _hip.i64_array(ul)), (None if lr is None else _hip.i64_array(lr))

  def h2d(self, host, ul=None, lr=None, staged=False):
    """Upload; returns host_consumed (None for the plain entry point).  The plain one is waited for."""
    host = np.ascontiguousarray(host, self.dtype)
    u, l = self._box(ul, lr)
    lib = _hip.lib()
    if staged:
      consumed = C.c_int32(-1)
      _hip.check(lib.sp_blob_h2d_staged(self.h, C.c_void_p(host.ctypes.data), u, l, _NULL, C.byref(consumed)))
      if not consumed.value:
        _hip.check(lib.sp_stream_synchronize(_NULL))
      return consumed.value
    _hip.check(lib.sp_blob_h2d(self.h, C.c_void_p(host.ctypes.data), u, l, _NULL))
    _hip.check(lib.sp_stream_synchronize(_NULL))
    return None

  def d2h(self, ul=None, lr=None, staged=False):
    shape = self.shape if ul is None else tuple(b - a for a, b in zip(ul, lr))
    out = np.full(int(np.prod(shape, dtype=np.int64)) * self.dtype.itemsize, 0x5B, np.uint8).view(self.dtype).reshape(shape)
    u, l = self._box(ul, lr)
    lib = _hip.lib()
    if staged:
      _hip.check(lib.sp_blob_d2h_staged(self.h, C.c_void_p(out.ctypes.data), u, l, _NULL))     # complete on return
    else:
      _hip.check(lib.sp_blob_d2h(self.h, C.c_void_p(out.ctypes.data), u, l, _NULL))
      _hip.check(lib.sp_stream_synchronize(_NULL))
    return out


def _blob_boxes(shape):
  """(kind, ul, lr) -- kind: 'whole', 'contiguous' (one byte range), 'proper' (staged through the box kernel), 'empty'."""
  nd = len(shape)
  full = tuple(shape)
  zero = (0,) * nd
  out = [('whole', None, None), ('whole', zero, full)]
  mid = tuple(n // 2 for n in shape)
  # a range of the first axis whose extent is not 1 (a run of rows; any range of a 1-d blob)
  k = next((i for i, n in enumerate(shape) if n > 2), None)
  if k is not None:
    ul = tuple(1 if i == k else 0 for i in range(nd))
    lr = tuple(shape[i] - 1 if i == k else shape[i] for i in range(nd))
    out.append(('contiguous', ul, lr))
  if nd >= 2 and shape[-1] > 3:
    # leading single indices, then a range of the last axis
    out.append(('contiguous', mid[:-1] + (1,), tuple(m + 1 for m in mid[:-1]) + (shape[-1] - 1,)))
    # a single cell
    out.append(('contiguous', mid, tuple(m + 1 for m in mid)))
  if nd >= 3:
    out.append(('contiguous', (mid[0],) + (min(1, shape[1] - 1),) + zero[2:], (mid[0] + 1,) + (shape[1],) + full[2:]))
  if nd >= 2 and all(n > 2 for n in shape):
    out.append(('proper', (1,) * nd, tuple(n - 1 for n in shape)))
    out.append(('proper', zero, full[:-1] + (shape[-1] - 1,)))                     # all but the last column
    out.append(('proper', zero[:-1] + (1,), full[:-1] + (2,)))                     # one column
  for a in range(nd):
    out.append(('empty', tuple(mid[i] if i == a else 0 for i in range(nd)), tuple(mid[i] if i == a else shape[i] for i in range(nd))))
  return out


_BLOB_SHAPES = [(37,), (9, 14), (5, 6, 7), (4, 1, 6), (1, 5, 6), (3, 4, 5, 6), (3, 1, 4, 5)]


def test_blob_boxes_are_classified_like_numpy():
  """The kinds the table above names are what NumPy says about the same slices (no GPU needed for this part, but it
  belongs with the table)."""
  for shape in _BLOB_SHAPES:
    a = np.zeros(shape, np.uint8)
    kinds = set()
    for kind, ul, lr in _blob_boxes(shape):
      v = a if ul is None else a[tuple(slice(x, y) for x, y in zip(ul, lr))]
      want = 'empty' if v.size == 0 else 'whole' if v.shape == a.shape else 'contiguous' if v.flags['C_CONTIGUOUS'] else 'proper'
      assert kind == want, (shape, kind, ul, lr)
      kinds.add(kind)
    assert kinds >= {'whole', 'contiguous', 'empty'} and ('proper' in kinds or 1 in shape or len(shape) == 1), shape


@pytest.mark.parametrize('es', [1, 2, 4, 8])
def test_blob_box_transfers(es):
  dt = np.dtype(_BLOB_DTYPES[es])
  failures = []
  for si, shape in enumerate(_BLOB_SHAPES):
    base = _random_values(dt, shape, si)
    for bi, (kind, ul, lr) in enumerate(_blob_boxes(shape)):
      box = tuple(slice(None) for _ in shape) if ul is None else tuple(slice(a, b) for a, b in zip(ul, lr))
      for staged in (False, True):
        what = '%s blob %s, %s box %s..%s, %s' % (dt, shape, kind, ul, lr, 'staged' if staged else 'plain')
        blob = Blob(shape, dt)
        blob.h2d(base)
        ref = base.copy()
        vals = _random_values(dt, ref[box].shape, 100 + bi)
        ref[box] = vals
        consumed = blob.h2d(vals, ul, lr, staged=staged)
        if staged and consumed != (1 if kind in ('whole', 'contiguous') else 0):
          failures.append(what + ': host_consumed = %d' % consumed)
        inside = np.zeros(shape, bool)
        inside[box] = True
        msg = (cc.first_difference(blob.d2h(staged=not staged), ref, inside, what + ' [whole blob read back]') or
               cc.first_difference(blob.d2h(ul, lr, staged=staged), vals, None, what + ' [box read back]') or
               cc.first_difference(blob.d2h(ul, lr, staged=not staged), vals, None, what + ' [box read back, other entry]'))
        if msg:
          failures.append(msg)
        blob.close()
  assert not failures, '%d:\n%s' % (len(failures), '\n'.join(failures[:20]))


def test_blob_staging_ring_consumes_the_host_buffer():
  """20 staged uploads from ONE host buffer that is overwritten as soon as each call returns: the ring of 8 pinned
  slots is gone round twice and every blob still holds its own values."""
  n = MiB // 2                                             # 2 MiB of float32 per upload
  blobs = [Blob((n,), np.float32) for _ in range(20)]
  values = [_random_values(np.float32, (n,), 300 + k) for k in range(20)]
  buf = np.empty(n, np.float32)
  lib = _hip.lib()
  for k, b in enumerate(blobs):
    buf[:] = values[k]
    consumed = C.c_int32(-1)
    _hip.check(lib.sp_blob_h2d_staged(b.h, C.c_void_p(buf.ctypes.data), None, None, _NULL, C.byref(consumed)))
    assert consumed.value == 1, k
    buf[:] = np.float32(-1.0)                              # the caller's buffer is its own again
  for k, b in enumerate(blobs):
    same(b.d2h(staged=bool(k % 2)), values[k], 'blob %d of 20' % k)
  # a range of a 1-d blob through the ring, at an odd offset
  big = Blob((3 * n + 5,), np.float32)
  base = _random_values(np.float32, (3 * n + 5,), 1)
  big.h2d(base)
  for k in range(10):
    buf[:] = values[k]
    assert big.h2d(buf, (k + 1,), (k + 1 + n,), staged=True) == 1
    base[k + 1:k + 1 + n] = values[k]
    buf[:] = 0
  same(big.d2h(), base, 'ranges of a 1-d blob through the ring')


def test_blob_staging_limit_and_fallback():
  lim = 4 * MiB
  for nbytes, want in ((lim, 1), (lim + 1, 0)):
    b = Blob((nbytes,), np.uint8)
    vals = cc.random_bytes(nbytes, nbytes % 7)
    assert b.h2d(vals, staged=True) == want, nbytes
    same(b.d2h(staged=True), vals, 'upload of %d bytes' % nbytes)
    same(b.d2h(), vals, 'upload of %d bytes, plain read' % nbytes)
    b.close()
  # a contiguous box above the limit and a proper box below it both fall back and still arrive
  b = Blob((3000, 1024), np.float32)
  base = _random_values(np.float32, (3000, 1024), 2)
  b.h2d(base)
  rows = _random_values(np.float32, (1025, 1024), 3)
  assert b.h2d(rows, (7, 0), (1032, 1024), staged=True) == 0
  base[7:1032] = rows
  cols = _random_values(np.float32, (3000, 3), 4)
  assert b.h2d(cols, (0, 5), (3000, 8), staged=True) == 0
  base[:, 5:8] = cols
  same(b.d2h(), base, 'fallbacks of the staged upload')
  same(b.d2h((0, 5), (3000, 8), staged=True), cols, 'proper box, staged read')
  same(b.d2h((7, 0), (1031, 1024), staged=True), base[7:1031], 'exactly 4 MiB of rows, staged read')


def test_blob_five_dimensions_and_refusals():
  lib = _hip.lib()
  shape = (2, 3, 4, 5, 6)
  b = Blob(shape, np.float32)
  base = _random_values(np.float32, shape, 1)
  for staged in (False, True):
    b.h2d(base, staged=staged)
    same(b.d2h(staged=staged), base, 'whole 5-d blob')
    vals = _random_values(np.float32, (1, 2, 4, 5, 6), 2 + staged)
    b.h2d(vals, (1, 1, 0, 0, 0), (2, 3, 4, 5, 6), staged=staged)              # contiguous: one byte range
    base[1:2, 1:3] = vals
    same(b.d2h(staged=staged), base, 'contiguous box of a 5-d blob')
    same(b.d2h((1, 1, 0, 0, 0), (2, 3, 4, 5, 6), staged=staged), vals, 'contiguous box of a 5-d blob, read')
  host = np.zeros((2, 3, 4, 5, 5), np.float32)
  p = C.c_void_p(host.ctypes.data)
  ul, lr = _hip.i64_array((0,) * 5), _hip.i64_array((2, 3, 4, 5, 5))
  consumed = C.c_int32(-1)
  for call in (lambda: lib.sp_blob_h2d(b.h, p, ul, lr, _NULL), lambda: lib.sp_blob_d2h(b.h, p, ul, lr, _NULL),
               lambda: lib.sp_blob_h2d_staged(b.h, p, ul, lr, _NULL, C.byref(consumed)),
               lambda: lib.sp_blob_d2h_staged(b.h, p, ul, lr, _NULL)):
    with pytest.raises(_hip.HipError, match=r'a proper box of a 5-d blob \(boxes are supported up to 4-d\)'):
      _hip.check(call())
  same(b.d2h(), base, 'a refused transfer wrote nothing')
  # boxes outside the blob
  m = Blob((9, 14), np.int16)
  hp = C.c_void_p(np.zeros((9, 14), np.int16).ctypes.data)
  for ul, lr in (((0, 0), (10, 14)), ((0, -1), (9, 14)), ((5, 0), (4, 14)), ((0, 0), (9, 15))):
    for call in (lambda: lib.sp_blob_h2d(m.h, hp, _hip.i64_array(ul), _hip.i64_array(lr), _NULL),
                 lambda: lib.sp_blob_d2h(m.h, hp, _hip.i64_array(ul), _hip.i64_array(lr), _NULL),
                 lambda: lib.sp_blob_h2d_staged(m.h, hp, _hip.i64_array(ul), _hip.i64_array(lr), _NULL, C.byref(consumed)),
                 lambda: lib.sp_blob_d2h_staged(m.h, hp, _hip.i64_array(ul), _hip.i64_array(lr), _NULL)):
      with pytest.raises(_hip.HipError, match='outside axis'):
        _hip.check(call())
  with pytest.raises(_hip.HipError, match='unknown blob handle'):
    _hip.check(lib.sp_blob_h2d(C.c_uint64(1 << 60), hp, None, None, _NULL))
  with pytest.raises(_hip.HipError, match='NULL host'):
    _hip.check(lib.sp_blob_h2d(m.h, None, None, None, _NULL))


@pytest.mark.parametrize('es', [1, 2, 4, 8])
def test_blob_slice_copy(es):
  lib = _hip.lib()
  dt = np.dtype(_BLOB_DTYPES[es])

  def copy(dst, dst_ul, src, src_ul, extent):
    return lib.sp_blob_slice_copy(dst.h, None if dst_ul is None else _hip.i64_array(dst_ul), src.h,
                                  None if src_ul is None else _hip.i64_array(src_ul), _hip.i64_array(extent), _NULL)

  # between blobs of different shapes, ranks 1 to 4
  for (dshape, sshape, dul, sul, ext) in (((37,), (50,), (3,), (11,), (30,)),
                                          ((9, 14), (20, 33), (2, 1), (5, 16), (6, 12)),
                                          ((9, 16), (20, 32), (1, 0), (4, 16), (8, 16)),          # the widened kernel
                                          ((5, 6, 7), (4, 9, 11), (1, 0, 2), (0, 3, 4), (3, 6, 5)),
                                          ((3, 4, 5, 6), (2, 6, 5, 9), (1, 1, 0, 1), (0, 2, 0, 3), (2, 3, 5, 4)),
                                          ((9, 14), (20, 33), (2, 1), (5, 16), (0, 12)),          # empty
                                          ((64, 70), (70, 64), None, None, (64, 64))):            # NULL origins
    a, s = _random_values(dt, dshape, 1), _random_values(dt, sshape, 2)
    dst, src = Blob(dshape, dt), Blob(sshape, dt)
    dst.h2d(a)
    src.h2d(s)
    _hip.check(copy(dst, dul, src, sul, ext))
    d0, s0 = dul or (0,) * len(ext), sul or (0,) * len(ext)
    dbox = tuple(slice(u, u + e) for u, e in zip(d0, ext))
    ref = a.copy()
    ref[dbox] = s[tuple(slice(u, u + e) for u, e in zip(s0, ext))]
    inside = np.zeros(dshape, bool)
    inside[dbox] = True
    cc.assert_same_bytes(dst.d2h(), ref, inside, '%s: %s <- %s, extent %s' % (dt, dshape, sshape, ext))
    same(src.d2h(), s, 'the source blob changed')
  # between disjoint boxes of ONE blob
  a = _random_values(dt, (40, 48), 3)
  one = Blob((40, 48), dt)
  one.h2d(a)
  _hip.check(copy(one, (20, 5), one, (1, 16), (19, 32)))
  ref = a.copy()
  ref[20:39, 5:37] = a[1:20, 16:48]
  same(one.d2h(), ref, 'disjoint boxes of one blob')
  # refusals
  other_rank, other_dtype = Blob((40,), dt), Blob((40, 48), np.int32 if es != 4 else np.int16)
  with pytest.raises(_hip.HipError, match='rank / dtype of the two blobs differ'):
    _hip.check(copy(one, (0,), other_rank, (0,), (4,)))
  with pytest.raises(_hip.HipError, match='rank / dtype of the two blobs differ'):
    _hip.check(copy(one, (0, 0), other_dtype, (0, 0), (4, 4)))
  small = Blob((10, 12), dt)
  small.h2d(np.zeros((10, 12), dt))
  for dul, sul, ext in (((0, 0), (0, 0), (11, 4)),         # outside the source
                        ((38, 0), (0, 0), (3, 4)),         # outside the destination
                        ((0, 45), (0, 0), (4, 4)), ((0, 0), (0, 9), (4, 4)), ((-1, 0), (0, 0), (4, 4)),
                        ((0, 0), (0, 0), (-1, 4))):
    with pytest.raises(_hip.HipError, match='box outside a blob'):
      _hip.check(copy(one, dul, small, sul, ext))
  same(one.d2h(), ref, 'a refused copy wrote nothing')
  five = Blob((2, 2, 2, 2, 2), dt)
  with pytest.raises(_hip.HipError, match='up to 4-d'):
    _hip.check(copy(five, None, five, None, (1, 1, 1, 1, 1)))
