"""What the prepared-operand path of the split-tier GEMM decides on the host, without a GPU: the size of an operand's
image buffer (sp_gemm_image_bytes) against its formula, and the policy of the backend's image cache
(backend_hip._GemmImageCache) against a stand-in `prepare` and arrays in host memory: sighting, keep on the second
sighting, reuse, a version bump by every kind of write, eviction under the byte budget, death with the storage.
tests/test_gemm_split_plan.py pins which shapes take the tier; nothing here may move those answers."""
import gc

import numpy as np
import pytest

from spartan_amd import _hip
from spartan_amd import devarray as D
from spartan_amd.backend_hip import _GemmImageCache


@pytest.mark.parametrize('side', [0, 1])
@pytest.mark.parametrize('rows,k', [(7681, 501), (8196, 501), (7969, 527), (1, 1), (3, 16), (3, 17), (8192, 8192)])
def test_image_bytes_formula(side, rows, k):
  # a 256-byte head, then three images of ceil(K / 16) k-tiles of `rows` rows of 16 bf16
  assert _hip.lib().sp_gemm_image_bytes(_hip.SP_F32, side, rows, k) == 256 + 3 * ((k + 15) // 16) * rows * 16 * 2


@pytest.mark.parametrize('dtype,side,rows,k', [(_hip.SP_F64, 0, 100, 100), (_hip.SP_F32, 0, 0, 100), (_hip.SP_F32, 1, 100, 0),
                                               (_hip.SP_F32, 0, -5, 100), (_hip.SP_F32, 2, 100, 100)])
def test_image_bytes_zero(dtype, side, rows, k):
  assert _hip.lib().sp_gemm_image_bytes(dtype, side, rows, k) == 0


def test_workspace_is_one_head_and_both_operands_images():
  lib = _hip.lib()
  m, n, k = 7681, 8196, 501
  images = sum(lib.sp_gemm_image_bytes(_hip.SP_F32, side, rows, k) - 256 for side, rows in ((0, m), (1, n)))
  assert lib.sp_gemm_split_workspace_bytes(_hip.SP_F32, m, n, k) == 512 + images


# ---- the cache's policy -----------------------------------------------------------------------------------------------
class _Handle(object):
  def __init__(self, x, side, nbytes):
    self.made_from, self.side, self.nbytes = x.numpy().copy(), side, nbytes


class _Prepare(object):
  """Stand-in for kernels.gemm_prepare: remembers what it was called with; a handle weighs `nbytes`."""

  def __init__(self, nbytes=100):
    self.calls, self.nbytes = [], nbytes

  def __call__(self, x, side):
    self.calls.append(side)                             # (not x: the stand-in must not keep the operand alive)
    return _Handle(x, side, self.nbytes)


def _host_array(shape=(8, 12), seed=0):
  return D.from_numpy(np.random.RandomState(seed).rand(*shape).astype(np.float32), storage_cls=D.HostStorage)


def test_sighting_keep_reuse():
  prep = _Prepare()
  cache = _GemmImageCache(prep, budget=1000)
  a = _host_array()
  assert cache.operand(a, 0) is None                    # first sighting: the product cuts, nothing is kept
  assert cache.stats == {'cuts': 1, 'reuses': 0, 'kept_bytes': 0, 'evictions': 0} and not prep.calls
  h = cache.operand(a, 0)                               # second: cut into a kept buffer
  assert h is not None and len(prep.calls) == 1
  assert cache.stats == {'cuts': 2, 'reuses': 0, 'kept_bytes': 100, 'evictions': 0}
  assert cache.operand(a, 0) is h and cache.operand(a, 0) is h and len(prep.calls) == 1
  assert cache.stats == {'cuts': 2, 'reuses': 2, 'kept_bytes': 100, 'evictions': 0}


def test_key_is_the_view_and_the_side():
  cache = _GemmImageCache(_Prepare(), budget=1000)
  a = _host_array()
  for _ in range(2):
    cache.operand(a, 0)
  kept = cache.operand(a, 0)
  assert kept is not None
  # another view of the same storage (an equal one made afresh is the same key), the other side, a transpose
  assert cache.operand(a[0:8, 0:12], 0) is kept
  assert cache.operand(a[1:8], 0) is None and cache.operand(a, 1) is None and cache.operand(a.T, 0) is None
  assert cache.operand(a[:, 0:8], 0) is None


@pytest.mark.parametrize('writer', ['upload', 'note_write', 'note_write_of_a_view', 'wrote'])
def test_a_write_moves_the_version_and_the_entry_goes(writer):
  prep = _Prepare()
  cache = _GemmImageCache(prep, budget=1000)
  a = _host_array()
  cache.operand(a, 0)
  old = cache.operand(a, 0)
  assert cache.operand(a, 0) is old
  if writer == 'upload':
    a.upload(np.ones(a.shape, np.float32))
  elif writer == 'note_write':
    D.note_write(a)
  elif writer == 'note_write_of_a_view':
    D.note_write(a[2:3, 4:5])
  else:
    cache.wrote(a[1:2])
    assert cache.stats['kept_bytes'] == 0                # (dropped at once, not at the next look)
  cuts = cache.stats['cuts']
  assert cache.operand(a, 0) is None                    # as if never seen: the product cuts the new bytes itself
  assert cache.stats['kept_bytes'] == 0 and cache.stats['cuts'] == cuts + 1
  new = cache.operand(a, 0)
  assert new is not None and new is not old and len(prep.calls) == 2
  assert np.array_equal(new.made_from, a.numpy())


def test_exported_storage_is_never_kept():
  cache = _GemmImageCache(_Prepare(), budget=1000)
  a = _host_array()
  cache.operand(a, 0)
  assert cache.operand(a, 0) is not None and cache.stats['kept_bytes'] == 100
  a.storage.version = -1 << 62                          # what __cuda_array_interface__ leaves behind
  for _ in range(3):
    assert cache.operand(a, 0) is None
  assert cache.stats['kept_bytes'] == 0 and cache.stats['cuts'] == 5 and not cache._entries      # (the kept buffer went too)


def test_eviction_is_least_recently_used_and_under_the_budget():
  cache = _GemmImageCache(_Prepare(nbytes=100), budget=250)
  arrays = [_host_array(seed=i) for i in range(3)]
  for x in arrays[:2]:
    cache.operand(x, 0)
    assert cache.operand(x, 0) is not None
  assert cache.stats['kept_bytes'] == 200 and cache.stats['evictions'] == 0
  cache.operand(arrays[0], 0)                           # arrays[1] is now the least recently used
  cache.operand(arrays[2], 0)
  assert cache.operand(arrays[2], 0) is not None
  assert cache.stats['kept_bytes'] == 200 and cache.stats['evictions'] == 1
  reuses = cache.stats['reuses']
  assert cache.operand(arrays[0], 0) is not None and cache.stats['reuses'] == reuses + 1
  assert cache.operand(arrays[1], 0) is None            # evicted: a first sighting again


def test_a_handle_over_the_budget_is_used_but_not_kept():
  cache = _GemmImageCache(_Prepare(nbytes=100), budget=50)
  a = _host_array()
  cache.operand(a, 0)
  assert cache.operand(a, 0) is not None and cache.stats['kept_bytes'] == 0
  assert cache.operand(a, 0) is not None and cache.stats['reuses'] == 0 and cache.stats['cuts'] == 3


def test_entries_die_with_their_storage():
  cache = _GemmImageCache(_Prepare(), budget=1000)
  a, b = _host_array(seed=1), _host_array(seed=2)
  for _ in range(2):
    cache.operand(a, 0)
    cache.operand(b, 0)
  assert cache.stats['kept_bytes'] == 200
  del a
  gc.collect()
  assert cache.stats['kept_bytes'] == 100
  del b
  gc.collect()
  assert cache.stats['kept_bytes'] == 0 and not cache._entries and not cache._storages


def test_switched_off_keeps_nothing():
  prep = _Prepare()
  cache = _GemmImageCache(prep, enabled=False)
  a = _host_array()
  assert [cache.operand(a, 0) for _ in range(3)] == [None] * 3 and not prep.calls
  assert cache.stats == {'cuts': 3, 'reuses': 0, 'kept_bytes': 0, 'evictions': 0}


def test_clear_gives_everything_back():
  cache = _GemmImageCache(_Prepare(), budget=1000)
  a = _host_array()
  cache.operand(a, 0)
  cache.operand(a, 0)
  cache.clear()
  assert cache.stats['kept_bytes'] == 0 and not cache._entries and not cache._storages
  assert cache.operand(a, 0) is None                    # a first sighting again


def test_no_room_for_a_kept_buffer_empties_the_cache_and_the_product_cuts():
  calls = []

  def prepare(x, side):
    calls.append(side)
    if len(calls) == 2:
      raise _hip.HipError('out of memory')
    return _Handle(x, side, 100)

  cache = _GemmImageCache(prepare, budget=1000)
  a, b = _host_array(seed=1), _host_array(seed=2)
  cache.operand(a, 0)
  assert cache.operand(a, 0) is not None and cache.stats['kept_bytes'] == 100
  cache.operand(b, 1)
  assert cache.operand(b, 1) is None and cache.stats['kept_bytes'] == 0 and not cache._entries


def test_launchers_note_what_they_write():
  """kernels._writes, which every launcher with a destination carries: the named arrays' storages move on before the
  launch, positional or by keyword, None skipped."""
  from spartan_amd import kernels
  seen = []

  @kernels._writes('out', 'extra')
  def launcher(src, out, extra=None):
    seen.append((src.storage.version, out.storage.version))
    return out

  src, out, extra = _host_array(seed=1), _host_array(seed=2), _host_array(seed=3)
  v0 = [t.storage.version for t in (src, out, extra)]      # (the upload that filled them has moved them already)
  assert launcher(src, out) is out and seen == [(v0[0], v0[1] + 1)]
  launcher(src, out=out[1:2], extra=extra)
  assert [t.storage.version for t in (src, out, extra)] == [v0[0], v0[1] + 2, v0[2] + 1]
  import inspect
  for name in ('update', 'slice_copy', 'gemm_f32', 'map_fused', 'reduce', 'stream_copy'):
    assert hasattr(getattr(kernels, name), '__wrapped__'), name
  assert list(inspect.signature(kernels.gemm_f32).parameters)[:3] == ['a', 'b', 'c']
