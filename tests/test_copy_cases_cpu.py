"""The data-movement case tables (tests/copy_cases.py) checked without a GPU: the references reproduce NumPy's own
slicing, the compare helper names a planted wrong byte in the box, in the guard and in the mask, every row reaches --
by the library's own host-side answer (sp_slice_copy_path / sp_update_path, the functions the launches ask) -- the
kernel it was written for, and every (path, element size, rank) cell the tables promise is reached by some row."""
import numpy as np
import pytest

from spartan_amd import _hip, kernels
from spartan_amd import devarray as D
from tests import copy_cases as cc


# ------------------------------------------------------------------------------------------------- the references
def test_copy_reference_reproduces_numpy_slicing():
  """Rows spelt a second time as ordinary NumPy slicing of ordinary arrays: the as_strided reference must agree."""
  rng = np.random.RandomState(11)
  for es in (1, 2, 4, 8):
    dt = cc.WORD[es]
    a = cc.random_words(es, 40 * 48, 5).reshape(40, 48)
    spelt = [
        ('box', (20, 16), (16, 1), (48, 1), 5 * 48 + 8, lambda a: a[5:25, 8:24]),
        ('step', (7, 6), (6, 1), (2 * 48, 3), 3 * 48 + 1, lambda a: a[3:17:2, 1:19:3]),
        ('reversed rows', (40, 48), (48, 1), (-48, 1), 39 * 48, lambda a: a[::-1]),
        ('reversed columns', (40, 48), (48, 1), (48, -1), 47, lambda a: a[:, ::-1]),
        ('transpose', (48, 40), (40, 1), (1, 48), 0, lambda a: a.T),
        ('transpose of every second row', (48, 20), (20, 1), (1, 96), 0, lambda a: a.T[:, ::2]),
        ('diagonal', (40,), (1,), (49,), 0, lambda a: a.diagonal()),
        ('broadcast row', (5, 48), (48, 1), (0, 1), 7 * 48, lambda a: np.broadcast_to(a[7], (5, 48))),
        ('scalar', (), (), (), 9 * 48 + 3, lambda a: a[9, 3]),
    ]
    for name, shape, dstr, sstr, origin, fn in spelt:
      n = int(np.prod(shape, dtype=np.int64))
      case = cc.CopyCase(name, es, shape, dstr, sstr, cc.GUARD, origin, n + 2 * cc.GUARD, a.size, 'box', False)
      dst = cc.pattern_words(es, case.dst_len)
      want, inside = cc.copy_expected(case, dst, a.reshape(-1))
      np.testing.assert_array_equal(want[cc.GUARD:cc.GUARD + n].reshape(shape), fn(a), err_msg='%s es=%d' % (name, es))
      np.testing.assert_array_equal(want[:cc.GUARD], dst[:cc.GUARD])
      np.testing.assert_array_equal(want[cc.GUARD + n:], dst[cc.GUARD + n:])
      assert inside.sum() == n and inside[cc.GUARD:cc.GUARD + n].all()
  # a strided DESTINATION against NumPy assignment, and the table's own rows against a per-element loop
  base = cc.pattern_words(4, 30 * 20)
  case = cc.CopyCase('into a step view', 4, (5, 4), (3 * 20, -2), (4, 1), 2 * 20 + 9, 0, base.size, 20, 'box', False)
  src = cc.random_words(4, 20, 1)
  want, inside = cc.copy_expected(case, base, src)
  ref = base.copy().reshape(30, 20)
  ref[2:17:3, 9:1:-2] = src.reshape(5, 4)
  np.testing.assert_array_equal(want.reshape(30, 20), ref)
  assert inside.sum() == 20
  small = [c for c in cc.COPY_CASES if not c.big and int(np.prod(c.shape, dtype=np.int64)) <= 600]
  for i in rng.choice(len(small), size=60, replace=False):
    case = small[i]
    dst, src = cc.copy_inputs(case, seed=int(i))
    want, inside = cc.copy_expected(case, dst, src)
    loop = dst.copy()
    for idx in np.ndindex(*case.shape):
      d = case.dst_origin + sum(k * s for k, s in zip(idx, case.dst_strides))
      s = case.src_origin + sum(k * s for k, s in zip(idx, case.src_strides))
      assert 0 <= d < case.dst_len and 0 <= s < case.src_len, case.name
      loop[d] = src[s]
    np.testing.assert_array_equal(want, loop, err_msg=case.name)


def test_every_copy_row_stays_inside_its_buffers_with_guards():
  for case in cc.COPY_CASES:
    dlo, dhi = cc._reach(case.shape, case.dst_strides)
    slo, shi = cc._reach(case.shape, case.src_strides)
    assert case.dst_origin + dlo >= cc.GUARD and case.dst_origin + dhi + cc.GUARD < case.dst_len + 1, case.name
    assert case.src_origin + slo >= cc.GUARD and case.src_origin + shi + cc.GUARD < case.src_len + 1, case.name
    assert case.dst_len * case.es <= 17 << 20 and case.src_len * case.es <= 17 << 20, case.name
    # no two cells of the box share a destination element (the expected result would depend on the order)
    if not case.big and all(n > 0 for n in case.shape):
      hits = np.zeros(case.dst_len, np.int32)
      view = cc._box_view(hits, case.dst_origin, case.shape, case.dst_strides)
      np.add.at(view, tuple(np.indices(case.shape).reshape(len(case.shape), -1)) if case.shape else (), 1)
      assert hits.max() == 1 and hits.sum() == int(np.prod(case.shape, dtype=np.int64)), case.name


def test_update_reference_reproduces_numpy_slicing():
  """Tile.merge spelt with plain slicing on plain arrays for a sample of rows (all ranks, all three dtype pairs)."""
  rows = [c for c in cc.UPDATE_CASES if not c.big]
  rng = np.random.RandomState(3)
  for i in list(rng.choice(len(rows), size=120, replace=False)) + [i for i, c in enumerate(rows) if 'eligible' in c.name]:
    case = rows[i]
    tb, mb, ub = cc.update_inputs(case, seed=int(i))
    tile, mask, upd = [x.copy() for x in cc.update_views(case, tb, mb, ub)]
    want_t, want_m, in_t, in_m = cc.update_expected(case, tb, mb, ub)
    got_t, got_m, _ = cc.update_views(case, want_t, want_m, ub)
    box = tuple(slice(a, b) for a, b in zip(case.ul, case.lr))
    ref = tile.copy()
    with np.errstate(all='ignore'):
      for idx in np.ndindex(*upd.shape):
        at = tuple(a + k for a, k in zip(case.ul, idx))
        was = {_hip.MASK_ALL_CLEAR: False, _hip.MASK_ALL_SET: True, _hip.MASK_ARRAY: mask[at] != 0}[case.mask_mode]
        if was and case.reducer == 'ADD':
          ref[at] = np.asarray(cc.nan_pinned_add(tile[at], upd[idx])).astype(case.tile_dtype)
        else:
          ref[at] = upd[idx].astype(case.tile_dtype)
    cc.assert_same_bytes(got_t, ref, None, case.name)
    refm = mask.copy()
    if case.with_mask:
      refm[box] = 1
    cc.assert_same_bytes(got_m, refm, None, case.name + ' (mask)')
    # the guards of the buffers are untouched and the box is what `inside` says
    n = tile.size
    t0 = cc.GUARD + case.tile_shift
    assert want_t[:t0].tobytes() == tb[:t0].tobytes() and want_t[t0 + n:].tobytes() == tb[t0 + n:].tobytes()
    assert in_t.sum() == upd.size and in_m.sum() == (upd.size if case.with_mask else 0)
    assert not in_t[:t0].any() and not in_t[t0 + n:].any()


def test_nan_plus_nan_is_pinned_to_what_numpys_contiguous_loop_gives():
  """IEEE 754 does not say whose payload NaN + NaN carries.  The merge reference pins it (copy_cases.nan_pinned_add:
  the second operand's, quieted); that is NumPy's own answer on contiguous arrays, and everywhere else the pinned
  add IS np.add."""
  for dt, bits, expo in ((np.float32, np.uint32, 0x7f800000), (np.float64, np.uint64, 0x7ff0000000000000)):
    rng = np.random.RandomState(1)
    n = 4099
    mant = (1 << np.finfo(dt).nmant) - 1
    nans = lambda seed: ((cc.random_bytes(n * np.dtype(dt).itemsize, seed).view(bits) & bits(mant)) | bits(1) |      # noqa: E731
                         bits(expo) | (cc.random_bytes(n * np.dtype(dt).itemsize, seed + 1).view(bits) & ~bits(mant) & ~bits(expo)))
    a, b = nans(1).view(dt), nans(3).view(dt)
    assert np.isnan(a).all() and np.isnan(b).all() and (a.view(bits) != b.view(bits)).all()
    with np.errstate(all='ignore'):
      cc.assert_same_bytes(cc.nan_pinned_add(a, b), np.add(a, b), None, 'NaN + NaN, contiguous %s' % np.dtype(dt))
      # strided operands and scalars: the pinned add gives the same bytes whatever the layout
      cc.assert_same_bytes(cc.nan_pinned_add(a[::2], b[::2]), np.add(a, b)[::2], None, 'NaN + NaN, strided')
      cc.assert_same_bytes(cc.nan_pinned_add(a[5], b[5]), np.add(a, b)[5], None, 'NaN + NaN, scalars')
      # one NaN, no NaN, every other bit pattern: plain np.add
      x, y = cc.random_bytes(n * np.dtype(dt).itemsize, 5).view(dt), cc.random_bytes(n * np.dtype(dt).itemsize, 6).view(dt)
      y[::3] = b[::3]
      x[::7] = a[::7]
      both = np.isnan(x) & np.isnan(y)
      assert both.any() and (np.isnan(x) ^ np.isnan(y)).any()
      got, ref = cc.nan_pinned_add(x, y), np.add(x, y)
      cc.assert_same_bytes(got, ref, None, 'random %s' % np.dtype(dt))
  # mixed widths: the update's NaN in the promoted type
  with np.errstate(all='ignore'):
    a64, b32 = nans(1).view(np.float64), np.float32([np.nan] * n)
    b32.view(np.uint32)[:] |= cc.random_bytes(4 * n, 9).view(np.uint32) & np.uint32(0x803fffff)
    cc.assert_same_bytes(cc.nan_pinned_add(a64, b32), np.add(a64, b32.astype(np.float64)), None, 'float64 + float32')
    assert cc.nan_pinned_add(np.int32([1, 2]), np.int64([3, 4])).tolist() == [4, 6]


# ------------------------------------------------------------------------------------------------- the compare helper
def test_compare_helper_names_a_planted_byte_in_box_guard_and_mask():
  case = next(c for c in cc.COPY_CASES if c.name == 'es4 rank 2 wide, padded rows')
  dst, src = cc.copy_inputs(case)
  want, inside = cc.copy_expected(case, dst, src)
  assert cc.first_difference(want.copy(), want, inside) is None
  in_box, in_guard = int(np.flatnonzero(inside)[3]), int(np.flatnonzero(~inside)[-1])
  for elem, word in ((in_box, 'inside the box'), (in_guard, 'in the guard')):
    for byte in range(case.es):
      got = want.copy()
      got.view(np.uint8)[elem * case.es + byte] ^= 0x01          # one bit of one byte
      msg = cc.first_difference(got, want, inside, 'dst')
      assert msg is not None and word in msg and 'element %d, byte %d' % (elem, byte) in msg, msg
      with pytest.raises(AssertionError, match=word):
        cc.assert_same_bytes(got, want, inside, 'dst')
  # a NaN whose payload differs is a difference (values would compare "both NaN")
  a = np.array([np.nan, 1.0], np.float32)
  b = a.copy()
  b.view(np.uint32)[0] ^= 1
  assert cc.first_difference(a, b) is not None and cc.first_difference(np.float32([0.0]), np.float32([-0.0])) is not None
  # merge: tile and mask each, inside the box and outside it
  case = next(c for c in cc.UPDATE_CASES if 'eligible' in c.name and c.mask_mode == _hip.MASK_ARRAY and c.reducer == 'ADD')
  tb, mb, ub = cc.update_inputs(case)
  want_t, want_m, in_t, in_m = cc.update_expected(case, tb, mb, ub)
  cc.assert_same_bytes(want_t.copy(), want_t, in_t, 'tile')
  for buf, inside, what in ((want_t, in_t, 'tile'), (want_m, in_m, 'mask')):
    for elem, word in ((int(np.flatnonzero(inside)[-1]), 'inside the box'), (int(np.flatnonzero(~inside)[0]), 'in the guard')):
      got = buf.copy()
      got.view(np.uint8)[elem * buf.dtype.itemsize] ^= 0x80
      with pytest.raises(AssertionError, match='%s: .*%s' % (what, word)):
        cc.assert_same_bytes(got, buf, inside, what)
  # a mask byte left at a non-zero value other than 1 is a difference
  got = want_m.copy()
  got[int(np.flatnonzero(in_m)[0])] = 2
  assert 'mask' in cc.first_difference(got, want_m, in_m, 'mask')


# ------------------------------------------------------------------------------------------------- the paths
def test_every_copy_row_reaches_the_path_it_names():
  for case in cc.COPY_CASES:
    assert cc.copy_path_of(case) == cc.copy_path_expected(case), case.name
    # the answer does not depend on WHERE the (16-byte aligned) buffers are
    assert cc.copy_path_of(case, cc.FAKE_BASE + 4096, cc.FAKE_BASE + 48) == cc.copy_path_expected(case), case.name
  # the second trips really are second trips: more work items than the grid holds
  grid = 256 * 8 * 256
  big = {c.name: c for c in cc.COPY_CASES if c.big}
  assert len(big) == 4
  for c in big.values():
    n = int(np.prod(c.shape, dtype=np.int64))
    if c.path == 'transpose':
      assert ((c.shape[0] + 63) // 64) * ((c.shape[1] + 63) // 64) == 8194 > 256 * 8 * 4
    else:
      assert n // (16 // c.es if c.path == 'wide' else 1) > grid


def test_every_copy_cell_is_reached():
  reached = set()
  for case in cc.COPY_CASES:
    path, word = cc.copy_path_of(case)
    reached.add((path, case.es, cc.copy_rank(case)))
  missing = [cell for cell in cc.COPY_CELLS if cell not in reached]
  assert not missing, missing
  assert ('transpose', 1, 2) not in reached and not [c for c in reached if c[0] == 'transpose' and c[2] != 2]
  # every transpose size pair, for every element size that has the kernel
  for es in (2, 4, 8):
    pairs = {(c.shape[1], c.shape[0]) for c in cc.COPY_CASES if c.es == es and c.path == 'transpose'}
    assert {(r, c) for r in (16, 17, 63, 64, 65, 129) for c in (16, 17, 63, 64, 65, 129)} <= pairs


def test_each_widening_condition_is_flipped_alone():
  """The 'miss' rows differ from their widened twin in ONE argument, and that argument alone changes the answer."""
  for es in (1, 2, 4, 8):
    rows = {c.name[len('es%d ' % es):]: c for c in cc.COPY_CASES if c.es == es}
    twin = rows['rank 2 wide, padded rows']
    assert cc.copy_path_of(twin) == ('wide', 16)
    for name in ('miss: inner extent', 'miss: dst outer stride', 'miss: src outer stride',
                 'miss: dst base off by one element', 'miss: src base off by one element',
                 'miss: dst inner stride 2', 'miss: src inner stride 2'):
      c = rows[name]
      changed = [f for f in ('shape', 'dst_strides', 'src_strides') if getattr(c, f) != getattr(twin, f)]
      changed += [f for f in ('dst_origin', 'src_origin') if getattr(c, f) % 16 != getattr(twin, f) % 16]
      assert len(changed) == 1, (name, changed)
      assert cc.copy_path_of(c) == ('box', es), name


def test_every_update_row_reaches_the_path_it_names():
  for case in cc.UPDATE_CASES:
    assert cc.update_path_of(case) == (case.cls, case.vec), case.name
  big = [c for c in cc.UPDATE_CASES if c.big]
  assert len(big) == 2
  for c in big:
    assert int(np.prod(cc.update_box_shape(c), dtype=np.int64)) // c.vec > 256 * 8 * 256


def test_every_update_cell_is_reached():
  reached = {(c.cls, cc.update_path_of(c)[1], len(c.tile_shape)) for c in cc.UPDATE_CASES}
  missing = [cell for cell in cc.UPDATE_CELLS if cell not in reached]
  assert not missing, missing
  # every reducer x mask mode at every rank, on the scalar kernel and (rank >= 1) on the vector kernel
  for nd in range(5):
    for vec in ((1,) if nd == 0 else (1, 4)):
      combos = {(c.reducer, c.mask_mode) for c in cc.UPDATE_CASES if len(c.tile_shape) == nd and c.vec == vec}
      assert len(combos) == 6, (nd, vec, combos)
  # each of the four conditions alone, for every vector width
  for cls in ('float', 'double', 'int64'):
    names = {c.name.split(': ', 1)[1] for c in cc.UPDATE_CASES if c.cls == cls and c.vec == 1 and 'break' in c.name}
    assert len(names) == 5, (cls, names)       # (the pointer condition is broken on either side)


def test_path_queries_refuse_what_the_launches_refuse():
  a = cc.FAKE_BASE
  with pytest.raises(_hip.HipError, match='ndim=5'):
    kernels.slice_copy_path(a, (1,) * 5, a, (1,) * 5, (1,) * 5, 4)
  with pytest.raises(_hip.HipError, match='elem_size=3'):
    kernels.slice_copy_path(a, (1,), a, (1,), (4,), 3)
  with pytest.raises(_hip.HipError, match='NULL'):
    kernels.slice_copy_path(0, (1,), a, (1,), (4,), 4)
  with pytest.raises(_hip.HipError, match='negative extent'):
    kernels.slice_copy_path(a, (1,), a, (1,), (-1,), 4)
  with pytest.raises(_hip.HipError, match='outside tile extent'):
    kernels.update_path(a, np.float32, (4, 4), (0, 0), (4, 5), a, np.float32)
  with pytest.raises(_hip.HipError, match='outside tile extent'):
    kernels.update_path(a, np.float32, (4, 4), (3, 0), (2, 4), a, np.float32)
  with pytest.raises(_hip.HipError, match='ndim=5'):
    kernels.update_path(a, np.float32, (1,) * 5, (0,) * 5, (1,) * 5, a, np.float32)
  with pytest.raises(_hip.HipError, match='NULL'):
    kernels.update_path(a, np.float32, (4,), (0,), (4,), 0, np.float32)
  # the class of a pair is NumPy's promotion (sp_merge_class), whatever the box
  for dst, src, cls in ((np.float16, np.int8, 'half'), (np.int16, np.float16, 'float'), (np.float32, np.int32, 'double'),
                        (np.uint8, np.bool_, 'int64'), (np.float64, np.float64, 'double')):
    assert kernels.update_path(a, dst, (8, 8), (0, 0), (8, 8), a, src)[0] == cls
  assert _hip.lib().sp_abi_version() == 1


# ------------------------------------------------------------------------------------------------- overlap
def test_overlap_test_of_paste_against_numpy():
  """HipBackend.paste copies its source first when D.may_overlap says so: the answer must be "yes" whenever NumPy
  sees shared memory, for views made every way the fuzz makes them (a "yes" too many costs a copy, never a result)."""
  from tests.test_devarray import _random_index, host
  rng = np.random.RandomState(17)
  a = np.arange(6 * 7 * 8, dtype=np.float32).reshape(6, 7, 8)
  d = host(a)
  said_no = 0
  for _ in range(600):
    i, j = _random_index(rng, a.shape), _random_index(rng, a.shape)
    if np.shares_memory(a[i], a[j]):
      assert D.may_overlap(d[i], d[j]), (i, j)
    else:
      said_no += not D.may_overlap(d[i], d[j])
  assert said_no > 20                       # disjoint slices are seen as disjoint (spans, so not all of them)
  assert D.may_overlap(d[1:], d[:-1]) and D.may_overlap(d, d.T) and D.may_overlap(d[::-1], d)
  assert not D.may_overlap(d[:3], d[3:]) and not D.may_overlap(d[0:0], d) and not D.may_overlap(d, host(a))
  assert D.element_span(d[::-1, ::-2, 3]) == (3, 5 * 56 + 6 * 8 + 3 + 1) and D.element_span(d[2:2]) is None
