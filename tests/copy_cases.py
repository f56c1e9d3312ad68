"""Case tables and plain NumPy references for the data-movement entry points: sp_slice_copy (box copy, box copy
widened to 16-byte words, LDS-tiled transpose) and sp_update (Tile.merge).  No GPU here: tests/test_copy_cases_cpu.py
checks the tables and the references themselves, tests/test_data_movement_gpu.py runs the rows on the device.

Every row names the kernel it was written for (`path`); the library's own host-side queries (sp_slice_copy_path /
sp_update_path, the functions the launches ask) say on the CPU whether the row still reaches it.  Source data are
random BYTES viewed as the element type (every bit pattern occurs: NaN payloads, -0.0, subnormals); destinations are
larger than what is written and pre-filled with a position-dependent pattern; every comparison is of bytes."""
import collections

import numpy as np
from numpy.lib.stride_tricks import as_strided

from spartan_amd import _hip

GUARD = 32                       # elements before and after everything a row touches (a multiple of 16: bases stay aligned)
FAKE_BASE = 1 << 32              # a 16-byte aligned "address" for the host-side path queries
WORD = {1: np.dtype(np.uint8), 2: np.dtype(np.uint16), 4: np.dtype(np.uint32), 8: np.dtype(np.uint64)}
# what the rows are held as on the device (uint64 is no tile dtype; the bytes are what is compared)
DEVICE_DTYPE = {1: np.dtype(np.uint8), 2: np.dtype(np.uint16), 4: np.dtype(np.uint32), 8: np.dtype(np.int64)}


# ------------------------------------------------------------------------------------------------- data and compare
def random_bytes(nbytes, seed):
  return np.frombuffer(np.random.RandomState(seed).bytes(int(nbytes)), np.uint8).copy()


def random_words(es, n, seed):
  """n elements of `es` bytes, every byte random."""
  return random_bytes(n * es, seed).view(WORD[es])


def pattern_words(es, n):
  """n elements of `es` bytes whose every byte depends on its position (what a destination holds before the call)."""
  b = ((np.arange(n * es, dtype=np.int64) * 131 + 7) % 251).astype(np.uint8)
  return b.view(WORD[es])


def first_difference(got, want, inside=None, what='buffer'):
  """None if the two arrays hold the same bytes; otherwise one line naming the first byte that differs, the element it
  belongs to and -- with `inside`, one bool per element: is it part of the box the call writes? -- whether that
  element lies inside the box or in the guard around it.  `what` names the buffer (the mask of a merge says 'mask')."""
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  if got.nbytes != want.nbytes:
    return '%s: %d bytes, expected %d' % (what, got.nbytes, want.nbytes)
  g, w = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
  bad = np.flatnonzero(g != w)
  if not bad.size:
    return None
  item = max(got.dtype.itemsize, 1)
  b = int(bad[0])
  e = b // item
  where = ''
  if inside is not None:
    ins = np.ascontiguousarray(inside).reshape(-1)
    assert ins.size * item == g.size, (ins.size, item, g.size)
    where = ', inside the box' if ins[e] else ', in the guard (outside the box)'
    n_in = int(np.count_nonzero(ins[np.unique(bad // item)]))
    where += '; %d differing elements inside the box, %d outside' % (n_in, np.unique(bad // item).size - n_in)
  return ('%s: %d of %d bytes differ; first at byte %d (element %d, byte %d of it)%s: got 0x%02x, expected 0x%02x'
          % (what, bad.size, g.size, b, e, b % item, where, g[b], w[b]))


def assert_same_bytes(got, want, inside=None, what='buffer'):
  msg = first_difference(got, want, inside, what)
  if msg is not None:
    raise AssertionError(msg)


# ------------------------------------------------------------------------------------------------- sp_slice_copy
CopyCase = collections.namedtuple('CopyCase', 'name es shape dst_strides src_strides dst_origin src_origin dst_len '
                                              'src_len path big')


def _reach(shape, strides):
  """(lowest, highest) element offset from the origin that a box of `shape` walking `strides` touches."""
  lo = hi = 0
  for n, s in zip(shape, strides):
    if n > 0:
      lo += min(0, (n - 1) * s)
      hi += max(0, (n - 1) * s)
  return lo, hi


def _round16(n):
  return (n + 15) // 16 * 16


def copy_case(name, es, shape, dst_strides, src_strides, path, dst_shift=0, src_shift=0, big=False):
  """A row: the box origin of each side sits GUARD elements (rounded to 16 elements, so that the origin is 16-byte
  aligned) behind the lowest element the box reaches, plus `*_shift` elements for the rows that want an origin off
  the alignment; each buffer ends GUARD elements behind the highest element reached."""
  shape, dst_strides, src_strides = tuple(shape), tuple(dst_strides), tuple(src_strides)
  assert len(shape) == len(dst_strides) == len(src_strides) and path in ('box', 'wide', 'transpose')
  dlo, dhi = _reach(shape, dst_strides)
  slo, shi = _reach(shape, src_strides)
  d0, s0 = _round16(GUARD - dlo) + dst_shift, _round16(GUARD - slo) + src_shift
  return CopyCase(name, es, shape, dst_strides, src_strides, d0, s0, d0 + dhi + 1 + GUARD, s0 + shi + 1 + GUARD, path, big)


def copy_inputs(case, seed=0):
  """(dst before the call, src): 1-d arrays of the unsigned word of the case's element size."""
  return pattern_words(case.es, case.dst_len), random_words(case.es, case.src_len, 1000 + seed)


def _box_view(buf, origin, shape, strides):
  es = buf.dtype.itemsize
  lo, hi = _reach(shape, strides)
  assert 0 <= origin + lo and origin + hi < buf.size, 'the box leaves its buffer'
  return as_strided(buf[origin:], shape, [s * es for s in strides])


def copy_expected(case, dst, src):
  """(dst after the call, which of its elements the box covers): NumPy's own strided assignment."""
  want = dst.copy()
  inside = np.zeros(dst.size, bool)
  if all(n > 0 for n in case.shape):
    _box_view(want, case.dst_origin, case.shape, case.dst_strides)[...] = \
        _box_view(src, case.src_origin, case.shape, case.src_strides)
    _box_view(inside, case.dst_origin, case.shape, case.dst_strides)[...] = True
  return want, inside


def copy_rank(case):
  return len(case.shape)


def _copy_table():
  rows = []
  add = lambda *a, **k: rows.append(copy_case(*a, **k))        # noqa: E731
  for es in (1, 2, 4, 8):
    p = 16 // es                   # elements per 16-byte word
    t = 'es%d ' % es
    # -- the narrow box kernel and the widened one at every rank
    add(t + 'rank 0', es, (), (), (), 'box')
    add(t + 'rank 1 narrow', es, (5,), (1,), (1,), 'box')
    add(t + 'rank 1 single element', es, (1,), (1,), (1,), 'box')
    add(t + 'rank 2 narrow, padded rows', es, (7, 5), (11, 1), (9, 1), 'box')
    add(t + 'rank 3 narrow', es, (3, 4, 5), (63, 9, 1), (40, 7, 1), 'box')
    add(t + 'rank 4 narrow', es, (2, 3, 4, 5), (400, 100, 11, 1), (300, 70, 9, 1), 'box')
    add(t + 'rank 1 wide', es, (3 * p,), (1,), (1,), 'wide')
    add(t + 'rank 2 wide, dense', es, (5, 2 * p), (2 * p, 1), (2 * p, 1), 'wide')
    add(t + 'rank 2 wide, padded rows', es, (5, 2 * p), (4 * p, 1), (3 * p, 1), 'wide')
    add(t + 'rank 3 wide', es, (3, 4, 2 * p), (16 * p, 3 * p, 1), (20 * p, 4 * p, 1), 'wide')
    add(t + 'rank 4 wide', es, (2, 3, 4, p), (60 * p, 16 * p, 3 * p, 1), (48 * p, 12 * p, 2 * p, 1), 'wide')
    add(t + 'rank 2 wide, more than one block', es, (130, 3 * p), (4 * p, 1), (3 * p, 1), 'wide')
    add(t + 'rank 2 narrow, more than one block', es, (37, 53), (59, 1), (53, 1), 'box')
    # -- rows that miss the widening by exactly ONE condition (their twin above, 'rank 2 wide, padded rows', takes it)
    add(t + 'miss: inner extent', es, (5, 2 * p + 1), (4 * p, 1), (3 * p, 1), 'box')
    add(t + 'miss: dst outer stride', es, (5, 2 * p), (4 * p + 1, 1), (3 * p, 1), 'box')
    add(t + 'miss: src outer stride', es, (5, 2 * p), (4 * p, 1), (3 * p + 1, 1), 'box')
    add(t + 'miss: dst base off by one element', es, (5, 2 * p), (4 * p, 1), (3 * p, 1), 'box', dst_shift=1)
    add(t + 'miss: src base off by one element', es, (5, 2 * p), (4 * p, 1), (3 * p, 1), 'box', src_shift=1)
    add(t + 'miss: dst inner stride 2', es, (5, 2 * p), (8 * p, 2), (3 * p, 1), 'box')
    add(t + 'miss: src inner stride 2', es, (5, 2 * p), (4 * p, 1), (8 * p, 2), 'box')
    add(t + 'miss: rank 3, dst stride of axis 0', es, (3, 4, 2 * p), (16 * p + 1, 3 * p, 1), (20 * p, 4 * p, 1), 'box')
    add(t + 'miss: rank 3, src stride of axis 1', es, (3, 4, 2 * p), (16 * p, 3 * p, 1), (20 * p, 4 * p + 1, 1), 'box')
    add(t + 'miss: rank 1, base off by one element on both sides', es, (3 * p,), (1,), (1,), 'box', dst_shift=1, src_shift=1)
    # -- strides as DevArray.__getitem__ / permute / diagonal produce them
    add(t + 'src step 2 and 3', es, (6, 7), (7, 1), (2 * 23, 3), 'box')
    add(t + 'dst step 2 and 3', es, (6, 7), (3 * 23, 2), (7, 1), 'box')
    add(t + 'src negative inner', es, (6, 7), (7, 1), (20, -1), 'box')
    add(t + 'dst negative inner', es, (6, 7), (20, -1), (7, 1), 'box')
    add(t + 'src negative outer', es, (6, 7), (7, 1), (-20, 1), 'box')
    add(t + 'dst negative outer', es, (6, 7), (-20, 1), (7, 1), 'box')
    add(t + 'both negative on every axis, rank 3', es, (3, 4, 5), (-63, -9, -1), (-40, -7, -1), 'box')
    add(t + 'wide with a negative outer stride on each side', es, (5, 2 * p), (-4 * p, 1), (-3 * p, 1), 'wide')
    add(t + 'src negative step 2 inner, rank 1', es, (9,), (1,), (-2,), 'box')
    add(t + 'broadcast rows (src outer stride 0)', es, (6, 7), (9, 1), (0, 1), 'box')
    add(t + 'broadcast rows, wide', es, (5, 2 * p), (4 * p, 1), (0, 1), 'wide')
    add(t + 'broadcast scalar (src strides 0, 0)', es, (6, 7), (9, 1), (0, 0), 'box')
    add(t + 'broadcast columns (src inner stride 0)', es, (6, 7), (9, 1), (1, 0), 'box')
    add(t + 'broadcast, rank 4', es, (2, 3, 4, 5), (60, 20, 5, 1), (0, 5, 0, 1), 'box')
    add(t + 'permuted axes, rank 3', es, (6, 4, 5), (20, 5, 1), (1, 30, 6), 'box')
    add(t + 'permuted axes, rank 4', es, (5, 2, 4, 3), (24, 12, 3, 1), (1, 60, 5, 20), 'box')
    add(t + 'permuted destination, rank 3', es, (6, 4, 5), (1, 30, 6), (20, 5, 1), 'box')
    add(t + 'small transpose (below 16: box kernel)', es, (7, 9), (9, 1), (1, 7), 'box')
    add(t + 'diagonal source, rank 1', es, (9,), (1,), (13 + 1,), 'box')
    add(t + 'diagonal destination, rank 1', es, (9,), (13 + 1,), (1,), 'box')
    add(t + 'diagonal of a 3-d source, rank 2', es, (4, 5), (5, 1), (42, 6 + 1), 'box')
    # -- empty boxes: nothing is written
    add(t + 'empty, rank 1', es, (0,), (1,), (1,), 'box')
    add(t + 'empty inner axis, rank 2', es, (3, 0), (4, 1), (4, 1), 'box')
    add(t + 'empty outer axis, rank 3', es, (0, 3, 4), (12, 4, 1), (12, 4, 1), 'box')
    # -- the 16-element threshold of the transpose path: 15 on either side takes the box kernel
    add(t + 'transpose 15 x 64 (box kernel)', es, (64, 15), (15, 1), (1, 64), 'box')
    add(t + 'transpose 64 x 15 (box kernel)', es, (15, 64), (64, 1), (1, 15), 'box')
    if es == 1:
      add(t + 'transpose 64 x 64 of bytes (box kernel)', es, (64, 64), (64, 1), (1, 64), 'box')
      add(t + 'transpose 65 x 17 of bytes (box kernel)', es, (17, 65), (65, 1), (1, 17), 'box')
      continue
    # -- the LDS-tiled transpose: src is R x C with leading dimension src_ld, dst is C x R with leading dimension dst_ld
    sizes = (16, 17, 63, 64, 65, 129)
    for i, R in enumerate(sizes):
      for j, C in enumerate(sizes):
        pad = (i + j) % 3            # dense; src_ld > C; dst_ld > R -- and (below) both
        src_ld, dst_ld = C + (3 if pad == 1 else 0), R + (5 if pad == 2 else 0)
        add(t + 'transpose %d x %d, src_ld %d, dst_ld %d' % (R, C, src_ld, dst_ld), es, (C, R), (dst_ld, 1), (1, src_ld),
            'transpose')
    add(t + 'transpose 65 x 129, src_ld > C and dst_ld > R', es, (129, 65), (65 + 7, 1), (1, 129 + 2), 'transpose')
    add(t + 'transpose 16 x 16, both padded by one', es, (16, 16), (17, 1), (1, 17), 'transpose')
    add(t + 'transpose of every second row (a.T[:, ::2] of a 34 x 40 array)', es, (40, 17), (17, 1), (1, 2 * 40), 'transpose')
    add(t + 'transpose of every third row, padded, 130 x 70', es, (70, 44), (50, 1), (1, 3 * 75), 'transpose')
    add(t + 'transposed source with inner step (a.T[::2]: box kernel)', es, (20, 34), (34, 1), (2, 40), 'box')
    add(t + 'transposed source, dst rows step 2 (box kernel)', es, (40, 34), (68, 2), (1, 40), 'box')
    add(t + 'transposed source, dst rows reversed', es, (40, 34), (-34, 1), (1, 40), 'box')
  # -- beyond the grid cap: the loops take a second trip
  add('second trip: narrow box of 1025 x 513 bytes', 1, (1025, 513), (519, 1), (513, 1), 'box', big=True)
  add('second trip: wide box of 1024 x 2052 fp32 (525312 words)', 4, (1024, 2052), (2056, 1), (2052, 1), 'wide', big=True)
  add('second trip: transpose of 16 x 524353 uint16 (8194 tiles)', 2, (524353, 16), (16, 1), (1, 524353), 'transpose', big=True)
  add('second trip: transpose of 524353 x 16 uint16 (8194 tiles)', 2, (16, 524353), (524353, 1), (1, 16), 'transpose', big=True)
  names = [r.name for r in rows]
  assert len(set(names)) == len(names)
  return rows


COPY_CASES = _copy_table()

# every (path, element size, rank) the table has to reach
COPY_CELLS = ([('box', es, r) for es in (1, 2, 4, 8) for r in range(5)] +
              [('wide', es, r) for es in (1, 2, 4, 8) for r in range(1, 5)] +
              [('transpose', es, 2) for es in (2, 4, 8)])


def copy_path_of(case, dst_base=FAKE_BASE, src_base=FAKE_BASE):
  """The path the LIBRARY takes for the row with buffers at these base addresses: ('box' | 'wide' | 'transpose' |
  'nothing', bytes per thread step)."""
  from spartan_amd import kernels
  word, transpose = kernels.slice_copy_path(dst_base + case.dst_origin * case.es, case.dst_strides,
                                            src_base + case.src_origin * case.es, case.src_strides, case.shape, case.es)
  if word == 0:
    return 'nothing', 0
  return ('transpose' if transpose else ('wide' if word == 16 and case.es != 16 else 'box')), word


def copy_path_expected(case):
  if any(n == 0 for n in case.shape):
    return 'nothing', 0
  return case.path, (16 if case.path == 'wide' else case.es)


# ------------------------------------------------------------------------------------------------- sp_update
UpdateCase = collections.namedtuple('UpdateCase', 'name tile_dtype upd_dtype tile_shape ul lr reducer mask_mode '
                                                  'with_mask tile_shift upd_shift cls vec big')
MASK_NAMES = {_hip.MASK_ALL_CLEAR: 'all clear', _hip.MASK_ALL_SET: 'all set', _hip.MASK_ARRAY: 'array'}
_CLS = {(np.float32, np.float32): ('float', 4), (np.float64, np.float32): ('double', 2), (np.int32, np.int64): ('int64', 2)}


def update_case(name, pair, tile_shape, ul, lr, reducer, mask_mode, vec, with_mask=True, tile_shift=0, upd_shift=0,
                big=False):
  cls, V = _CLS[pair]
  assert vec in (0, 1, V) and (with_mask or mask_mode != _hip.MASK_ARRAY)
  return UpdateCase('%s <- %s %s, mask %s%s: %s' % (np.dtype(pair[0]), np.dtype(pair[1]), reducer, MASK_NAMES[mask_mode],
                                                    '' if with_mask else ' (no mask array)', name),
                    np.dtype(pair[0]), np.dtype(pair[1]), tuple(tile_shape), tuple(ul), tuple(lr), reducer, mask_mode,
                    with_mask, tile_shift, upd_shift, cls, vec, big)


def update_box_shape(case):
  return tuple(b - a for a, b in zip(case.ul, case.lr))


def update_inputs(case, seed=0):
  """(tile, mask, update) before the call, each inside a 1-d buffer with GUARD elements (of its own type) on both
  sides plus the row's shift: returns the three BUFFERS; update_views() cuts the arrays out of them.  Tile and
  update are random bytes; the mask holds 0 / non-zero bytes (1, 2 and 255 all mean "written")."""
  n_tile = int(np.prod(case.tile_shape, dtype=np.int64))
  n_upd = int(np.prod(update_box_shape(case), dtype=np.int64))
  tile = random_bytes((2 * GUARD + case.tile_shift + n_tile) * case.tile_dtype.itemsize, 2000 + seed).view(case.tile_dtype)
  upd = random_bytes((2 * GUARD + case.upd_shift + n_upd) * case.upd_dtype.itemsize, 3000 + seed).view(case.upd_dtype)
  mask = np.random.RandomState(4000 + seed).choice(np.array([0, 0, 0, 1, 1, 2, 255], np.uint8), size=2 * GUARD + n_tile)
  return tile, mask.astype(np.uint8), upd


def update_views(case, tile_buf, mask_buf, upd_buf):
  """(tile, mask, update) as arrays of the row's shapes: views of the three buffers."""
  n_tile = int(np.prod(case.tile_shape, dtype=np.int64))
  box = update_box_shape(case)
  n_upd = int(np.prod(box, dtype=np.int64))
  t0, u0 = GUARD + case.tile_shift, GUARD + case.upd_shift
  return (tile_buf[t0:t0 + n_tile].reshape(case.tile_shape), mask_buf[GUARD:GUARD + n_tile].reshape(case.tile_shape),
          upd_buf[u0:u0 + n_upd].reshape(box))


def update_expected(case, tile_buf, mask_buf, upd_buf):
  """(tile buffer, mask buffer, which tile ELEMENTS of the tile buffer the box covers, the same for the mask buffer)
  after the call: Tile.merge in NumPy (the slicing of test_update_reducers_dtypes_masks) -- cells whose mask said
  "written" get reducer(old, update) computed in NumPy's promoted dtype and cast to the tile's, the others
  update.astype(tile dtype); mask bytes of the box become 1 (when the call is given a mask array); nothing else
  changes."""
  want_tile, want_mask = tile_buf.copy(), mask_buf.copy()
  tile, mask, upd = update_views(case, want_tile, want_mask, upd_buf)
  in_tile, in_mask = np.zeros(tile_buf.size, bool), np.zeros(mask_buf.size, bool)
  box = tuple(slice(a, b) for a, b in zip(case.ul, case.lr))
  if all(n > 0 for n in update_box_shape(case)):
    region = tile[box + (Ellipsis,)]             # (a view for a 0-d tile as well)
    written = {_hip.MASK_ALL_CLEAR: np.zeros(region.shape, bool), _hip.MASK_ALL_SET: np.ones(region.shape, bool),
               _hip.MASK_ARRAY: mask[box] != 0}[case.mask_mode]
    with np.errstate(all='ignore'):
      u = upd.astype(case.tile_dtype)
      merged = u if case.reducer == 'NONE' else np.asarray(nan_pinned_add(region, upd)).astype(case.tile_dtype)
    region[...] = np.where(written, merged, u)
    update_views(case, in_tile, in_mask, upd_buf)[0][box] = True
    if case.with_mask:                     # (without a mask array the call has no mask to write)
      mask[box] = 1
      update_views(case, in_tile, in_mask, upd_buf)[1][box] = True
  return want_tile, want_mask, in_tile, in_mask


def nan_pinned_add(old, upd):
  """np.add(old, upd) with the one cell IEEE 754 leaves open spelt out: where BOTH operands are NaN the result is the
  second operand's NaN (in the promoted type), quieted.  That is what NumPy's contiguous add loop gives on x86-64
  (tests/test_copy_cases_cpu.py checks that it does); its strided and scalar loops give the first operand's, so
  without this line the expected bytes would depend on the memory layout of the reference's own operands."""
  res = np.add(old, upd)
  if res.dtype.kind == 'f':
    o, u = np.asarray(old).astype(res.dtype), np.asarray(upd).astype(res.dtype)
    both = np.isnan(o) & np.isnan(u)
    if both.any():
      bits = np.dtype('u%d' % res.dtype.itemsize)
      quiet = bits.type(1) << bits.type(np.finfo(res.dtype).nmant - 1)
      res = np.array(res, copy=True)
      res.view(bits)[both] = u.view(bits)[both] | quiet
  return res


def _positions(shape):
  """(name, ul, lr) of the boxes every rank is tried at."""
  nd = len(shape)
  if nd == 0:
    return [('whole 0-d tile', (), ())]
  out = [('whole tile', (0,) * nd, shape),
         ('first cell', (0,) * nd, (1,) * nd),
         ('last cell', tuple(n - 1 for n in shape), shape)]
  mid = tuple(n // 2 for n in shape)
  if nd >= 2:
    out.append(('one row', (mid[0],) + (0,) * (nd - 1), (mid[0] + 1,) + shape[1:]))
    out.append(('one column', (0,) * (nd - 1) + (mid[-1],), shape[:-1] + (mid[-1] + 1,)))
  out.append(('inner box', tuple(min(1, n - 1) for n in shape), tuple(max(n - 1, 1) for n in shape)))
  for a in range(nd):
    ul = tuple(mid[i] if i == a else 0 for i in range(nd))
    lr = tuple(mid[i] if i == a else shape[i] for i in range(nd))
    out.append(('empty on axis %d' % a, ul, lr))
  return out


def _update_table():
  rows = []
  add = lambda *a, **k: rows.append(update_case(*a, **k))        # noqa: E731
  f32, f64f32, i32i64 = (np.float32, np.float32), (np.float64, np.float32), (np.int32, np.int64)
  modes = (_hip.MASK_ALL_CLEAR, _hip.MASK_ALL_SET, _hip.MASK_ARRAY)
  combos = [(r, m) for r in ('NONE', 'ADD') for m in modes]
  # -- every rank, every box position, every reducer x mask mode (odd extents: the scalar kernel)
  shapes = {0: (), 1: (13,), 2: (6, 9), 3: (3, 5, 7), 4: (2, 3, 5, 3)}
  for nd, shape in shapes.items():
    for pname, ul, lr in _positions(shape):
      empty = any(b == a for a, b in zip(ul, lr))
      for reducer, mode in combos:
        add('rank %d, %s' % (nd, pname), f32, shape, ul, lr, reducer, mode, 0 if empty else 1)
    add('rank %d, whole tile' % nd, f32, shape, (0,) * nd, shape, 'ADD', _hip.MASK_ALL_SET, 1, with_mask=False)
    add('rank %d, whole tile' % nd, f32, shape, (0,) * nd, shape, 'NONE', _hip.MASK_ALL_CLEAR, 1, with_mask=False)
  # -- the vector kernel at every rank that has one
  for nd, shape, ul, lr in ((1, (24,), (4,), (20,)), (2, (5, 12), (1, 4), (4, 12)), (3, (3, 4, 8), (1, 1, 0), (3, 3, 8)),
                            (4, (2, 3, 2, 8), (0, 1, 0, 4), (2, 3, 2, 8))):
    for reducer, mode in combos:
      add('rank %d, vector box' % nd, f32, shape, ul, lr, reducer, mode, 4)
  # -- per vector width: one eligible row and rows that break exactly ONE of the four conditions
  for pair in (f32, f64f32, i32i64):
    V = _CLS[pair][1]
    for reducer, mode in combos:
      add('eligible', pair, (6, 4 * V), (1, V), (5, 3 * V), reducer, mode, V)
      add('break: innermost extent', pair, (6, 4 * V), (1, V), (5, 3 * V - 1), reducer, mode, 1)
      add('break: offset of the box origin', pair, (6, 4 * V), (1, V + 1), (5, 3 * V + 1), reducer, mode, 1)
      add('break: outer stride of the tile', pair, (6, 4 * V + 1), (0, V), (5, 3 * V), reducer, mode, 1)
      add('break: tile pointer off 16 bytes', pair, (6, 4 * V), (1, V), (5, 3 * V), reducer, mode, 1, tile_shift=1)
      add('break: update pointer off 16 bytes', pair, (6, 4 * V), (1, V), (5, 3 * V), reducer, mode, 1, upd_shift=1)
  # -- beyond the grid cap: the loops take a second trip
  add('second trip: scalar box of 1025 x 513 in a 1030 x 520 tile', f32, (1030, 520), (3, 5), (1028, 518), 'ADD',
      _hip.MASK_ARRAY, 1, big=True)
  add('second trip: vector box of 1024 x 2052 (525312 vectors) in a 1026 x 2056 tile', f32, (1026, 2056), (1, 4),
      (1025, 2056), 'ADD', _hip.MASK_ARRAY, 4, big=True)
  names = [r.name for r in rows]
  assert len(set(names)) == len(names)
  return rows


UPDATE_CASES = _update_table()

# every (class, vector width, rank) the table has to reach; 0 = an empty box, nothing launched
UPDATE_CELLS = ([('float', 1, r) for r in range(5)] + [('float', 4, r) for r in range(1, 5)] +
                [('float', 0, r) for r in range(1, 5)] +
                [('double', 2, 2), ('double', 1, 2), ('int64', 2, 2), ('int64', 1, 2)])


def update_path_of(case, tile_base=FAKE_BASE, upd_base=FAKE_BASE):
  """The path the LIBRARY takes for the row with tile and update BUFFERS at these base addresses: (class, width)."""
  from spartan_amd import kernels
  return kernels.update_path(tile_base + (GUARD + case.tile_shift) * case.tile_dtype.itemsize, case.tile_dtype,
                             case.tile_shape, case.ul, case.lr,
                             upd_base + (GUARD + case.upd_shift) * case.upd_dtype.itemsize, case.upd_dtype)
