"""Prepared operands of the split-tier GEMM (kernels.gemm_prepare, gemm_f32(prepared_a=, prepared_b=)), the backend's
image cache behind HipBackend.dot, and the K-split pipeline's use of both.  The one bar everywhere is BIT EQUALITY with
the unprepared / uncached call in the same process -- which is what tests/test_gemm_split_*.py pin.

Shapes: E1 and E2 of tests/test_gemm_split_edges_gpu.py.  Two cases had to be stated differently from the issue:
  * rows [33, 7200) of E1's A give M = 7167, which the (unmoved) plan leaves on the fp32 tier -- with N = 8196 and
    K = 501 it takes M in 7169 .. 7681 --, so the row view is rows [33, 7233): 7200 rows, still an odd start that is no
    multiple of the cut's 32-row blocks and an end inside the operand;
  * a tile is a contiguous array, and E1's K = 501 gives it a row pitch the tier's layout refuses (ld % 4 != 0): the
    cache would never be asked.  The sp.dot cases use E4 (7936, 8196, 512), the nearest pinned shape a tile can hold."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from spartan_amd import _hip  # noqa: E402
from tests import gemm_split_child as child  # noqa: E402
from tests.test_gemm_split_edges_gpu import SHAPES, _selected, pads_of  # noqa: E402


def _bits(x):
  return np.ascontiguousarray(x).view(np.uint32)


def _same(got, want, what):
  diff = int(np.count_nonzero(_bits(got) != _bits(want)))
  print('%s: %d of %d elements differ' % (what, diff, want.size))
  return diff == 0


def _host(name, seed):
  m, n, k = SHAPES[name]
  rng = np.random.RandomState(seed)
  return (rng.uniform(-1, 1, (m, k)).astype(np.float32), rng.uniform(-1, 1, (k, n)).astype(np.float32),
          rng.uniform(-1, 1, (m, n)).astype(np.float32))


@pytest.fixture(scope='module')
def operands():
  """{name: (a, b, c0 on the host -- read-only --, a and b on the device with the padded pitches of the edge tests)}"""
  out = {}
  for i, name in enumerate(('E1', 'E2')):
    a, b, c0 = _host(name, 20261019 + i)
    for x in (a, b, c0):
      x.setflags(write=False)
    pads = pads_of(name)
    out[name] = (a, b, c0, child.padded(a, pads[0]), child.padded(b, pads[1]))
  return out


def _cut_launches():
  """Cut kernels launched by this process so far, counted by the library where it launches them."""
  return _hip.lib().sp_gemm_cut_launches()


def _gemm(da, db, c0, pad, accumulate, **prepared):
  """c0 (+)= da . db; asserts that the product launched one cut kernel per operand that came without images."""
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  c = child.padded(c0, pad)
  before = _cut_launches()
  kernels.gemm_f32(da, db, c, accumulate=accumulate, **prepared)
  assert _cut_launches() - before == 2 - len(prepared), sorted(prepared)
  D.synchronize()
  return c.numpy()


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('name', ['E1', 'E2'])
def test_prepared_equals_unprepared(operands, name, accumulate):
  from spartan_amd import kernels
  assert _selected(*SHAPES[name])
  _, _, c0, da, db = operands[name]
  pad = pads_of(name)[2]
  want = _gemm(da, db, c0, pad, accumulate)
  ha, hb = kernels.gemm_prepare(da, 0), kernels.gemm_prepare(db, 1)
  ok = [_same(_gemm(da, db, c0, pad, accumulate, **kw), want, '%s accumulate=%s %s' % (name, accumulate, sorted(kw)))
        for kw in ({'prepared_a': ha}, {'prepared_b': hb}, {'prepared_a': ha, 'prepared_b': hb})]
  assert all(ok)
  assert _same(_gemm(da, db, c0, pad, accumulate), want, 'unprepared again')


def test_row_view_and_column_view_of_prepared_operands(operands):
  from spartan_amd import kernels
  m, n, k = SHAPES['E1']
  _, _, c0, da, db = operands['E1']
  pad = pads_of('E1')[2]
  lib = _hip.lib()
  r0, r1 = 33, 7233
  assert lib.sp_gemm_split_workspace_bytes(_hip.SP_F32, r1 - r0, n, k) > 0
  ha = kernels.gemm_prepare(da, 0)
  want = _gemm(da[r0:r1], db, c0[r0:r1], pad, False)
  assert _same(_gemm(da[r0:r1], db, c0[r0:r1], pad, False, prepared_a=ha.view(r0, r1)), want, 'rows [33, 7233) of A')
  c0_, c1_ = 36, 7996
  assert lib.sp_gemm_split_workspace_bytes(_hip.SP_F32, m, c1_ - c0_, k) > 0
  hb = kernels.gemm_prepare(db, 1)
  want = _gemm(da, db[:, c0_:c1_], c0[:, c0_:c1_], pad, True)
  assert _same(_gemm(da, db[:, c0_:c1_], c0[:, c0_:c1_], pad, True, prepared_b=hb.view(c0_, c1_)), want,
               'columns [36, 7996) of B')
  assert _same(_gemm(da, db[:, c0_:c1_], c0[:, c0_:c1_], pad, True, prepared_a=ha, prepared_b=hb.view(c0_, c1_)), want,
               'columns [36, 7996) of B, A prepared too')
  with pytest.raises(ValueError):
    ha.view(0, m + 1)
  with pytest.raises(ValueError):      # a handle of another shape is refused, not read
    kernels.gemm_f32(da[r0:r1], db, child.padded(c0[r0:r1], pad), prepared_a=ha)


def test_each_operand_has_its_own_window_flag(operands):
  from spartan_amd import kernels
  m, n, k = SHAPES['E1']
  a, b, c0, da, db = operands['E1']
  pads = pads_of('E1')
  clean = _gemm(da, db, c0, pads[2], False)
  ha, hb = kernels.gemm_prepare(da, 0), kernels.gemm_prepare(db, 1)

  a_sub = a.copy()
  a_sub[m - 1, k - 1] = np.float32(2.0 ** -130)             # a subnormal: outside the window, the fp32 tier computes C
  da_sub = child.padded(a_sub, pads[0])
  want = _gemm(da_sub, db, c0, pads[2], False)
  assert not np.array_equal(_bits(want), _bits(clean))       # (the fp32 tier's bits, not the split tier's)
  assert _same(_gemm(da_sub, db, c0, pads[2], False, prepared_a=kernels.gemm_prepare(da_sub, 0)), want,
               'subnormal in A, A prepared, B raw')

  b_inf = b.copy()
  b_inf[k - 1, n - 1] = np.inf
  db_inf = child.padded(b_inf, pads[1])
  want = _gemm(da, db_inf, c0, pads[2], False)
  assert _same(_gemm(da, db_inf, c0, pads[2], False, prepared_b=kernels.gemm_prepare(db_inf, 1)), want,
               'Inf in B, B prepared, A raw')
  # the flags raised above live in those operands' own buffers: clean operands are not touched by them
  assert _same(_gemm(da, db, c0, pads[2], False, prepared_a=ha, prepared_b=hb), clean, 'clean, both prepared')
  assert _same(_gemm(da, db_inf, c0, pads[2], False, prepared_a=ha), want, 'Inf in raw B, A prepared')
  assert _same(_gemm(da, db, c0, pads[2], False, prepared_a=ha), clean, 'clean again, A prepared')


# ---- the cache behind HipBackend.dot ----------------------------------------------------------------------------------
E4 = SHAPES['E4']


@pytest.fixture()
def hip_ctx():
  import spartan_amd as sp
  ctx = sp.initialize('hip', num_workers=1)
  yield sp, ctx
  sp.shutdown()


def _images_bytes(m, n, k):
  lib = _hip.lib()
  return lib.sp_gemm_image_bytes(_hip.SP_F32, 0, m, k), lib.sp_gemm_image_bytes(_hip.SP_F32, 1, n, k)


def _uncached(da, db):
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  c = D.empty((da.shape[0], db.shape[1]), np.float32)
  kernels.gemm_f32(da, db, c)
  return c.numpy()


def test_cache_through_dot_on_one_tile(hip_ctx):
  sp, ctx = hip_ctx
  be = ctx.backend
  m, n, k = E4
  assert _selected(m, n, k)
  rng = np.random.RandomState(7)
  a, b = rng.uniform(-1, 1, (m, k)).astype(np.float32), rng.uniform(-1, 1, (k, n)).astype(np.float32)
  A, B = sp.from_numpy(a, tile_hint=a.shape), sp.from_numpy(b, tile_hint=b.shape)      # one tile each
  A.force(), B.force()
  s0 = be.gemm_image_stats
  r1 = sp.dot(A, B).glom()
  s1 = be.gemm_image_stats
  assert (s1['cuts'] - s0['cuts'], s1['reuses'] - s0['reuses'], s1['kept_bytes']) == (2, 0, 0)
  r2 = sp.dot(A, B).glom()
  s2 = be.gemm_image_stats
  assert (s2['cuts'] - s1['cuts'], s2['reuses'] - s1['reuses'], s2['kept_bytes']) == (2, 0, sum(_images_bytes(m, n, k)))
  launched = _cut_launches()
  r3 = sp.dot(A, B).glom()
  assert _cut_launches() == launched      # no cut kernel at all
  s3 = be.gemm_image_stats
  assert (s3['cuts'] - s2['cuts'], s3['reuses'] - s2['reuses'], s3['kept_bytes']) == (0, 2, s2['kept_bytes'])
  assert _same(r2, r1, 'call 2 (cut into kept buffers)') and _same(r3, r1, 'call 3 (reuse)')
  del A, B
  gc.collect()
  sp.from_numpy(np.zeros((2, 2), np.float32))      # (tiles of dead arrays go back when the next array is made)
  gc.collect()
  assert be.gemm_image_stats['kept_bytes'] == 0


def _warm(be, da, db):
  """Two products: both operands are kept afterwards."""
  be.dot(da, db)
  be.dot(da, db)
  assert be.gemm_image_stats['kept_bytes'] == sum(_images_bytes(da.shape[0], db.shape[1], da.shape[1]))


def _e4_operands(seed):
  from spartan_amd import devarray as D
  m, n, k = E4
  rng = np.random.RandomState(seed)
  return (rng, D.from_numpy(rng.uniform(-1, 1, (m, k)).astype(np.float32)),
          D.from_numpy(rng.uniform(-1, 1, (k, n)).astype(np.float32)))


def _check_writers(be, da, db, writers):
  """For each (name, side written, write()): with both operands kept, write, then the next product has the bits of
  the uncached call on the new data, cuts the written operand again (one cut kernel) and reuses the other."""
  for what, side, write in writers:
    _warm(be, da, db)
    before_host = (da if side == 0 else db).numpy()
    write()
    assert not np.array_equal(before_host, (da if side == 0 else db).numpy()), what      # (the writer did write)
    s0, launched = be.gemm_image_stats, _cut_launches()
    got = be.dot(da, db).numpy()
    s1 = be.gemm_image_stats
    assert _cut_launches() - launched == 1, what
    assert _same(got, _uncached(da, db), 'after %s' % what)
    assert (s1['cuts'] - s0['cuts'], s1['reuses'] - s0['reuses']) == (1, 1), what


def test_every_backend_writer_voids_the_kept_images(hip_ctx):
  import scipy.sparse
  from spartan_amd import devarray as D
  _, ctx = hip_ctx
  be = ctx.backend
  m, n, k = E4
  rng, da, db = _e4_operands(8)
  patch = D.from_numpy(rng.uniform(-1, 1, (4, k)).astype(np.float32))
  x, y = D.from_numpy(rng.uniform(-1, 1, (256, 16)).astype(np.float32)), D.from_numpy(rng.uniform(-1, 1, (16, 256)).astype(np.float32))
  sparse_update = scipy.sparse.random(8, k, density=0.25, format='csr', dtype=np.float32, random_state=rng)
  _check_writers(be, da, db, [
      ('__setitem__', 0, lambda: da.__setitem__((slice(5, 9), slice(3, 40)), 2.5)),
      ('fill', 0, lambda: da[7000:7001].fill(0.75)),
      ('upload', 0, lambda: da[m - 4:m].upload(rng.uniform(-1, 1, (4, k)).astype(np.float32))),
      ('paste', 0, lambda: be.paste(da, (slice(100, 104), slice(0, k)), patch)),
      ('update_box', 0, lambda: be.update_box(da, (200, 0), (204, k), patch, np.add, _hip.MASK_ALL_SET, None)),
      ('gemm_into out', 1, lambda: be.gemm_into(x, y, db[0:256, 4:260])),
      # a sparse update that lands on a dense tile (Tile.update -> sparse_scatter, mode 1: add)
      ('sparse_scatter', 0, lambda: be.sparse_scatter(da, (300, 0), sparse_update, 1, None)),
  ])
  del da, db
  gc.collect()
  assert be.gemm_image_stats['kept_bytes'] == 0


class _CopyTransport(object):
  """Same-process stand-in for a World transport: every receiving array gets `src`'s bytes by a bare device copy
  (the library call itself, so that nothing but World's own bookkeeping can have noted the write)."""
  name = 'copy'

  def __init__(self, src):
    self.src = src

  def _fill(self, dst):
    from spartan_amd import devarray as D
    assert dst.is_contiguous() and dst.nbytes <= self.src.nbytes
    _hip.check(_hip.lib().sp_stream_copy_wg(dst.data_ptr(), self.src.data_ptr(), dst.nbytes, 0, D.current_stream().ptr))

  def exchange(self, sends, recvs, async_=False):
    for _, t in recvs:
      self._fill(t)

  def all_gather_into(self, out, tensor, async_=False):
    self._fill(out)

  def reduce_scatter(self, out, inp, reducer, async_=False):
    self._fill(out)

  def all_reduce(self, tensor, reducer):
    self._fill(tensor)

  def reduce(self, tensor, dst, reducer):
    self._fill(tensor)

  def broadcast(self, tensor, src):
    self._fill(tensor)


def test_transfers_and_export_void_the_kept_images(hip_ctx):
  """The receiving arrays of every World primitive, and an array exported through __cuda_array_interface__."""
  from spartan_amd import comm
  from spartan_amd import devarray as D
  _, ctx = hip_ctx
  be = ctx.backend
  m, n, k = E4
  rng, da, db = _e4_operands(11)
  src = D.from_numpy(rng.uniform(-1, 1, (8, k)).astype(np.float32))
  other = D.from_numpy(rng.uniform(-1, 1, (4, k)).astype(np.float32))
  world = comm.World(rank=0, size=2, transport=_CopyTransport(src), control=object())
  rows = iter(range(400, 4000, 100))
  recv = lambda: da[next(rows):][:4]      # noqa: E731  (four whole rows of A: a contiguous receiving array)
  _check_writers(be, da, db, [
      ('exchange', 0, lambda: world.exchange([(1, other)], [(1, recv())])),
      ('exchange_async', 0, lambda: world.exchange_async([(1, other)], [(1, recv())])),
      ('all_gather_into', 0, lambda: world.all_gather_into(recv(), other)),
      ('all_gather_into_async', 0, lambda: world.all_gather_into_async(recv(), other)),
      ('reduce_scatter', 0, lambda: world.reduce_scatter(recv(), src, 'ADD')),
      ('reduce_scatter_async', 0, lambda: world.reduce_scatter_async(recv(), src, 'ADD')),
      ('all_reduce', 0, lambda: world.all_reduce(recv(), 'ADD')),
      ('reduce', 0, lambda: world.reduce(recv(), 0, 'ADD')),
      ('broadcast', 0, lambda: world.broadcast(recv(), 1)),
  ])
  # exported: another library may write these bytes at any time, so B is never kept again -- here the "other library"
  # is the bare copy, which nothing notes
  _warm(be, da, db)
  assert db.__cuda_array_interface__['data'][0] == db.data_ptr()
  kept_a = _images_bytes(m, n, k)[0]
  for i in range(3):
    _CopyTransport(src)._fill(db.reshape(-1)[i * 4096:][:8 * k])
    s0, launched = be.gemm_image_stats, _cut_launches()
    got = be.dot(da, db).numpy()
    s1 = be.gemm_image_stats
    assert _cut_launches() - launched == 1 and (s1['cuts'] - s0['cuts'], s1['reuses'] - s0['reuses']) == (1, 1)
    assert _same(got, _uncached(da, db), 'after export and an unseen write, call %d' % (i + 1))
    assert s1['kept_bytes'] == kept_a


def test_trim_pool_gives_the_kept_images_back(hip_ctx):
  from spartan_amd import devarray as D
  _, ctx = hip_ctx
  be = ctx.backend
  _, da, db = _e4_operands(12)
  want = _uncached(da, db)
  _warm(be, da, db)
  D.trim_pool()
  assert be.gemm_image_stats['kept_bytes'] == 0
  assert _same(be.dot(da, db).numpy(), want, 'after trim_pool')


def test_budget_smaller_than_two_operands_evicts(hip_ctx):
  _, ctx = hip_ctx
  be = ctx.backend
  m, n, k = E4
  _, da, db = _e4_operands(9)
  want = _uncached(da, db)
  be._gemm_images.budget = max(_images_bytes(m, n, k)) + 1
  for i in range(4):
    assert _same(be.dot(da, db).numpy(), want, 'call %d under a one-operand budget' % (i + 1))
    assert be.gemm_image_stats['kept_bytes'] <= be._gemm_images.budget
  assert be.gemm_image_stats['evictions'] >= 1


# ---- the users that prepare for themselves ----------------------------------------------------------------------------
def test_dot_chunked_cuts_a_once(hip_ctx):
  """a (E4's A) times B arriving as two column chunks of E4's width: a is cut once, not once per chunk."""
  from spartan_amd import devarray as D
  from spartan_amd import kernels
  from spartan_amd.array import distarray
  _, ctx = hip_ctx
  be = ctx.backend
  m, n, k = E4
  assert _selected(m, n, k)
  rng, da, _ = _e4_operands(13)
  chunks = [D.from_numpy(rng.uniform(-1, 1, (k, n)).astype(np.float32)) for _ in range(2)]
  want = D.empty((m, 2 * n), np.float32)
  launched = _cut_launches()
  for i, t in enumerate(chunks):
    kernels.gemm_f32(da, t, want[:, i * n:(i + 1) * n])
  assert _cut_launches() - launched == 4
  rhs = distarray.ChunkedWhole((k, 2 * n), np.float32, [(i * n, (i + 1) * n, t, None, None) for i, t in enumerate(chunks)])
  launched = _cut_launches()
  got = be.dot_chunked(da, rhs)
  assert _cut_launches() - launched == 3      # a once, each chunk of B once
  assert _same(got.numpy(), want.numpy(), 'dot_chunked with a prepared')
  assert be.gemm_image_stats['kept_bytes'] == 0


def test_ksplit_pipeline_cuts_the_slab_once(hip_ctx):
  """Rank 0 of 2 with same-process stand-in transports (plain device copies).  Slab 15360 x 512, two chunks of 8196
  columns.  Every product takes the split tier -- the own-block and row-block products of chunk 0 (7680, 8196, 512)
  and the whole-slab product of chunk 1 (15360, 8196, 512) --, so the row view of the slab's images and chunk 0's
  prepared b_chunk reach the split kernel.  Cut kernels, counted where the library launches them:
    without preparation  own block 2 + row block 2 + chunk 1 2                                              = 6
    with                 b_chunk 0 once, own block's rows of the slab once (before the blocks land), the slab
                         once, row block none, chunk 1's b_chunk once                                       = 4"""
  from spartan_amd import devarray as D
  import importlib
  dot_mod = importlib.import_module('spartan_amd.expr.dot')      # (spartan_amd.expr.dot the attribute is the dot() builder)
  _, ctx = hip_ctx
  be = ctx.backend
  p, me, mb, kb, nc = 2, 0, 7680, 512, 8196
  n = 2 * nc
  assert _selected(mb, nc, kb) and _selected(p * mb, nc, kb)
  rng = np.random.RandomState(10)
  a_full = rng.uniform(-1, 1, (p * mb, p * kb)).astype(np.float32)
  my_a = D.from_numpy(a_full[me * mb:(me + 1) * mb])
  my_b = D.from_numpy(rng.uniform(-1, 1, (kb, n)).astype(np.float32))
  blocks = {j: D.from_numpy(a_full[j * mb:(j + 1) * mb, me * kb:(me + 1) * kb]) for j in range(p) if j != me}

  def exchange(sends, recvs):
    for j, dst in recvs:
      be.paste(dst, (slice(0, mb), slice(0, kb)), blocks[j])
    return None

  def reduce_scatter(out, part):
    be.paste(out, (slice(0, mb), slice(0, nc)), part[me * mb:(me + 1) * mb])
    return None

  def run(prepare):
    s0, launched = be.gemm_image_stats, _cut_launches()
    r = dot_mod.ksplit_pipeline(be, p, me, my_a, my_b, np.dtype(np.float32), exchange, reduce_scatter, nc, prepare=prepare)
    return r.numpy(), be.gemm_image_stats['cuts'] - s0['cuts'], _cut_launches() - launched

  want, cuts, launched = run(False)
  assert (cuts, launched) == (0, 6)
  got, cuts, launched = run(True)
  assert _same(got, want, 'ksplit_pipeline with the slab prepared')
  assert (cuts, launched) == (2, 4)      # the stats count the two prepared operands: the slab and chunk 0's b_chunk
  assert be.gemm_image_stats['kept_bytes'] == 0
