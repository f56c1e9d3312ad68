"""Pythonic launchers over the C-ABI (spartan_amd/_hip.py) for tile blobs in HBM.

Operands are device arrays (spartan_amd/devarray.py: views of blobs the library's tile store owns); anything else
that can say where its bytes live in HBM -- `data_ptr()`, `shape`, `stride()`, `dtype` -- is accepted as well, so
a test may hand in memory from another allocator.  Launches go to devarray.current_stream().  No torch here.
"""
import ctypes as C
import functools
import inspect

import numpy as np

from . import _hip, devarray, tile_checks
from ._hip import check
from .devarray import Event  # noqa: F401  (bench.py / tools time launches with it)

_KNOWN = {n: np.dtype(n) for n in ('float32', 'float64', 'int32', 'int64', 'bool', 'uint8', 'int8', 'int16', 'uint16',
                                     'uint32', 'float16')}


def np_dtype_of(t):
  """NumPy dtype of a device operand (a DevArray carries one; foreign tensors name theirs, e.g. 'torch.float32')."""
  dt = t.dtype
  if isinstance(dt, np.dtype):
    return dt
  name = str(dt).split('.')[-1]
  if name not in _KNOWN:
    raise TypeError('dtype %s is not supported by the HIP tile backend' % (dt,))
  return _KNOWN[name]


def _stream():
  return devarray.current_stream().ptr


def _require_device(*tensors):
  for t in tensors:
    if t is not None and not getattr(t, 'is_cuda', False):
      raise _hip.HipError('HIP tile kernels need device (HBM) operands; got %s' % (type(t).__name__,))


def _elsize(t):
  return t.element_size() if hasattr(t, 'element_size') else t.itemsize


def _p(t):
  """Where `t` lives in HBM as a pointer argument; NULL for None."""
  return C.c_void_p(None if t is None else t.data_ptr())


def _writes(*names):
  """Decorator of a launcher whose parameters `names` are arrays the kernel writes: each one that is given has its
  storage's version moved on (devarray.note_write) before the launch, so that whatever was derived from the old bytes --
  the backend's GEMM images -- is void whoever calls the launcher.  For an array made a line earlier this is one integer
  increment."""
  def deco(fn):
    params = list(inspect.signature(fn).parameters)
    where = [(n, params.index(n)) for n in names]

    @functools.wraps(fn)
    def launcher(*args, **kw):
      for n, i in where:
        t = args[i] if i < len(args) else kw.get(n)
        if t is not None:
          devarray.note_write(t)
      return fn(*args, **kw)
    return launcher
  return deco


def _dtypes(*tensors):
  """The dtypes of the operands of a launcher, in their order, for its tile_checks function (None is skipped)."""
  return [np_dtype_of(t) for t in tensors if t is not None]


class Workspace(object):
  """Grow-only scratch blob for reduction partials (one per device)."""

  def __init__(self):
    self.buf = None

  def get(self, nbytes, device=None):
    if self.buf is None or self.buf.numel() < nbytes:
      self.buf = devarray.empty((max(int(nbytes), 1 << 20),), np.uint8)
    return self.buf


_ws = Workspace()


@_writes('out')
def map_fused(prog, inputs, out):
  """Launch the fused map `prog` over dense tensors; `out` is written."""
  _require_device(out, *inputs)
  ptrs = _hip.ptr_array([t.data_ptr() for t in inputs])
  check(_hip.lib().sp_map_fused(C.byref(prog), ptrs, C.c_void_p(out.data_ptr()), _stream()))
  return out


_reduce_ws_bytes = {}


@_writes('out')
def reduce(prog, inputs, red_op, outer, axis_len, inner, out):
  _require_device(out, *inputs)
  lib = _hip.lib()
  key = (prog.cls, outer, axis_len, inner)
  need = _reduce_ws_bytes.get(key)
  if need is None:                         # (a pure function of the plan's geometry: asked once per shape)
    if len(_reduce_ws_bytes) > 4096:
      _reduce_ws_bytes.clear()
    need = _reduce_ws_bytes[key] = lib.sp_reduce_workspace_bytes(prog.cls, outer, axis_len, inner)
  ws = _ws.get(need, out.device)
  ptrs = _hip.ptr_array([t.data_ptr() for t in inputs])
  check(lib.sp_reduce(C.byref(prog), ptrs, _hip.RED[red_op] if isinstance(red_op, str) else red_op,
                      outer, axis_len, inner, C.c_void_p(out.data_ptr()),
                      _hip.sp_dtype(np_dtype_of(out)), C.c_void_p(ws.data_ptr()), ws.numel(), _stream()))
  return out


def reduce_warm(prog, inputs, red_op, outer, axis_len, inner, out_dtype):
  """What the first reduce() of this program would set up besides the launch: the partials' workspace at its size."""
  need = _hip.lib().sp_reduce_workspace_bytes(prog.cls, outer, axis_len, inner)
  _ws.get(need)


@_writes('out_idx', 'out_val')
def argreduce(prog, inputs, which, outer, axis_len, inner, index_offset, nan_index, out_idx, out_val=None):
  _require_device(out_idx, out_val, *inputs)
  lib = _hip.lib()
  need = lib.sp_argreduce_workspace_bytes(prog.cls, outer, axis_len, inner)
  ws = _ws.get(need, out_idx.device)
  ptrs = _hip.ptr_array([t.data_ptr() for t in inputs])
  assert np_dtype_of(out_idx) == np.int64
  check(lib.sp_argreduce(C.byref(prog), ptrs, which, outer, axis_len, inner, int(index_offset),
                         int(nan_index), C.c_void_p(out_idx.data_ptr()),
                         C.c_void_p(out_val.data_ptr() if out_val is not None else 0),
                         C.c_void_p(ws.data_ptr()), ws.numel(), _stream()))
  return out_idx


@_writes('dst')
def update(dst, ul, lr, src, reducer, mask_mode, mask=None):
  """Tile.merge: dst[ul:lr] = merge(dst[ul:lr], src) with the tile's mask state."""
  _require_device(dst, src, mask)
  nd = dst.dim()
  check(_hip.lib().sp_update(
      C.c_void_p(dst.data_ptr()), _hip.sp_dtype(np_dtype_of(dst)), _hip.i64_array(dst.shape), nd,
      _hip.i64_array(ul), _hip.i64_array(lr), C.c_void_p(src.data_ptr()), _hip.sp_dtype(np_dtype_of(src)),
      _hip.REDUCER[reducer] if isinstance(reducer, str) else reducer, mask_mode,
      C.c_void_p(mask.data_ptr() if mask is not None else 0), _stream()))
  return dst


@_writes('dst')
def slice_copy(dst, dst_offset, dst_strides, src, src_offset, src_strides, shape):
  """Strided box copy between two blobs of the same element size (strides/offsets in elements)."""
  _require_device(dst, src)
  es = _elsize(dst)
  assert es == _elsize(src)
  nd = len(shape)
  check(_hip.lib().sp_slice_copy(
      C.c_void_p(dst.data_ptr() + int(dst_offset) * es), _hip.i64_array(dst_strides),
      C.c_void_p(src.data_ptr() + int(src_offset) * es), _hip.i64_array(src_strides),
      _hip.i64_array(shape), nd, es, _stream()))
  return dst


def slice_copy_path(dst_ptr, dst_strides, src_ptr, src_strides, shape, elem_size):
  """Which kernel slice_copy would launch for a box at these ADDRESSES (integers; host code, nothing is read or
  launched): (bytes one thread step moves -- the element size, 16 when widened, 0 for an empty box --, whether the
  LDS-tiled transpose kernel is taken).  Raises what the launch would raise."""
  word, transpose = C.c_int32(0), C.c_int32(0)
  check(_hip.lib().sp_slice_copy_path(
      C.c_void_p(int(dst_ptr)), _hip.i64_array(dst_strides), C.c_void_p(int(src_ptr)), _hip.i64_array(src_strides),
      _hip.i64_array(shape), len(shape), int(elem_size), C.byref(word), C.byref(transpose)))
  return word.value, bool(transpose.value)


_MERGE_CLASS = {_hip.SP_F16: 'half', _hip.SP_F32: 'float', _hip.SP_F64: 'double', _hip.SP_I64: 'int64'}


def update_path(dst_ptr, dst_dtype, dst_shape, ul, lr, src_ptr, src_dtype):
  """Which kernel update would launch for a tile and an update at these ADDRESSES (integers; host code, nothing is
  read or launched): (compute class -- 'half' (float arithmetic rounded to half), 'float', 'double' or 'int64' --,
  elements per thread step: 4, 2 or 1, 0 for an empty box).  Raises what the launch would raise."""
  cls, vec = C.c_int32(0), C.c_int32(0)
  check(_hip.lib().sp_update_path(
      C.c_void_p(int(dst_ptr)), _hip.sp_dtype(dst_dtype), _hip.i64_array(dst_shape), len(dst_shape), _hip.i64_array(ul),
      _hip.i64_array(lr), C.c_void_p(int(src_ptr)), _hip.sp_dtype(src_dtype), C.byref(cls), C.byref(vec)))
  return _MERGE_CLASS[cls.value], vec.value


class GemmImages(object):
  """One fp32 GEMM operand cut into the split tier's bf16 images (gemm_prepare): `buf` holds the operand's own window
  flag and the three images of all `img_rows` rows; the handle stands for rows [row0, row0 + rows) of them.  `event`
  was recorded on `stream` behind the cut: a product on another stream waits for it (gemm_f32 does).  The images are
  a snapshot: whoever keeps a handle across a write into the operand has to cut again."""
  __slots__ = ('buf', 'side', 'img_rows', 'K', 'row0', 'rows', 'event', 'stream')

  def __init__(self, buf, side, img_rows, K, row0, rows, event, stream):
    self.buf, self.side, self.img_rows, self.K = buf, side, img_rows, K
    self.row0, self.rows, self.event, self.stream = row0, rows, event, stream

  nbytes = property(lambda self: self.buf.numel())

  def view(self, r0, r1):
    """The images of rows [r0, r1) of this handle's operand (side 1: of its columns): nothing is cut again."""
    r0, r1 = int(r0), int(r1)
    if not 0 <= r0 < r1 <= self.rows:
      raise ValueError('rows [%d, %d) of a prepared operand of %d rows' % (r0, r1, self.rows))
    return GemmImages(self.buf, self.side, self.img_rows, self.K, self.row0 + r0, r1 - r0, self.event, self.stream)


def gemm_preparable(x, side):
  """Can `x` be cut by gemm_prepare: a 2-D fp32 device tensor that meets the split tier's layout for that side?"""
  if not getattr(x, 'is_cuda', False) or x.dim() != 2 or np_dtype_of(x) != np.float32:
    return False
  r, c = x.shape
  if r < 1 or c < 1 or r > 2147483647 or c > 2147483647 or (c > 1 and x.stride(1) != 1):
    return False
  ld = x.stride(0) if r > 1 else c
  return ld >= c and ld % 4 == 0 and x.data_ptr() % 16 == 0 and (256 if side == 0 else 16) * ld < (1 << 30)


def gemm_takes_split(M, N, K):
  """Does the fp32 product [M][K] . [K][N] run on the split tier (given operands that meet its layout)?"""
  return _hip.lib().sp_gemm_split_workspace_bytes(_hip.SP_F32, int(M), int(N), int(K)) > 0


def gemm_cut_launches():
  """How many cut kernels (one per operand cut, into a workspace or into a buffer) this process has launched."""
  return int(_hip.lib().sp_gemm_cut_launches())


def gemm_prepare(x, side):
  """Cut the fp32 operand `x` of a product once -- side 0: the left one, [M][K]; side 1: the right one, [K][N] -- into
  a buffer of its own (sp_gemm_cut), for any number of gemm_f32(..., prepared_a= / prepared_b=) calls while `x` keeps
  its bytes.  Returns a GemmImages.  Nothing remembers the handle: the caller owns it."""
  if side not in (0, 1) or not gemm_preparable(x, side):
    raise ValueError('gemm_prepare: side %r of a %s %s tensor with strides %s cannot be cut'
                     % (side, tuple(x.shape), x.dtype, tuple(x.stride())))
  lib = _hip.lib()
  rows, K = (x.shape[0], x.shape[1]) if side == 0 else (x.shape[1], x.shape[0])
  nbytes = lib.sp_gemm_image_bytes(_hip.SP_F32, side, rows, K)
  buf = devarray.empty((nbytes,), np.uint8)
  check(lib.sp_gemm_cut(side, _p(x), x.stride(0) if x.shape[0] > 1 else x.shape[1], rows, K, _p(buf), nbytes, _stream()))
  stream = devarray.current_stream()
  return GemmImages(buf, side, rows, K, 0, rows, Event().record(stream), stream)


def _prepared(h, side, rows, K, dt):
  """The (buffer, rows it was cut with, first row taken) arguments of a prepared operand; (NULL, 0, 0) for None."""
  if h is None:
    return C.c_void_p(0), 0, 0
  if dt != _hip.SP_F32 or h.side != side or h.rows != rows or h.K != K:
    raise ValueError('gemm_f32: the prepared operand (side %d, %d x %d) is not side %d of this fp32 product (%d x %d)'
                     % (h.side, h.rows, h.K, side, rows, K))
  if h.stream is not devarray.current_stream():
    devarray.current_stream().wait_event(h.event)
  return C.c_void_p(h.buf.data_ptr()), h.img_rows, h.row0


@_writes('c')
def gemm_f32(a, b, c, accumulate=False, prepared_a=None, prepared_b=None):
  """c (+)= a . b for 2-D row-major fp32 (or, all three, fp64) tensors (inner stride 1).  prepared_a / prepared_b:
  gemm_prepare's handle of `a` / `b` (or a view() of one for a row block of a / a column block of b): where the
  split tier runs, that operand is not cut again; where it does not, the handle is ignored.  The bits do not depend on
  it.  Nothing is cached here: without a handle every call cuts."""
  _require_device(a, b, c)
  adt = np_dtype_of(a)
  assert adt == np_dtype_of(b) == np_dtype_of(c) and adt in (np.float32, np.float64)
  lib = _hip.lib()
  dt = _hip.SP_F32 if adt == np.float32 else _hip.SP_F64
  M, K = a.shape
  K2, N = b.shape
  assert K == K2 and tuple(c.shape) == (M, N), (a.shape, b.shape, c.shape)
  assert a.stride(1) == 1 and b.stride(1) == 1 and c.stride(1) == 1
  pa, a_rows, a_row0 = _prepared(prepared_a, 0, M, K, dt)
  pb, b_rows, b_row0 = _prepared(prepared_b, 1, N, K, dt)
  need = lib.sp_gemm_workspace_bytes(dt, M, N, K)         # > 0: few output tiles, long contraction -> split-K
  if prepared_a is None and prepared_b is None:
    need = max(need, lib.sp_gemm_split_workspace_bytes(dt, M, N, K))   # > 0: the operand images of the bf16 split tier
  elif lib.sp_gemm_split_workspace_bytes(dt, M, N, K):    # the head, and the images of the side that comes raw
    need = max(need, 512 + sum(lib.sp_gemm_image_bytes(dt, side, rows, K) - 256
                               for side, rows, h in ((0, M, prepared_a), (1, N, prepared_b)) if h is None))
  ws = _ws.get(need, a.device) if need else None
  check(lib.sp_gemm_ws_images(dt, C.c_void_p(a.data_ptr()), a.stride(0) if M > 1 else max(K, 1), pa, a_rows, a_row0,
                              C.c_void_p(b.data_ptr()), b.stride(0) if K > 1 else max(N, 1), pb, b_rows, b_row0,
                              C.c_void_p(c.data_ptr()), c.stride(0) if M > 1 else max(N, 1),
                              M, N, K, 1 if accumulate else 0, C.c_void_p(ws.data_ptr() if need else 0),
                              ws.numel() if need else 0, _stream()))
  return c


def _rowdot_operands(x, w, y, out):
  """(n, d, ldx, ldy, workspace) of the one-pass rowdot kernels, or None when the operands do not meet their layout."""
  _require_device(x, w, out)
  n, d = x.shape
  need = _hip.lib().sp_rowdot_colsum_workspace_bytes(n, d) if n else 256
  ldx = x.stride(0) if n > 1 else d
  if (not need or x.stride(1) != 1 or ldx % 4 or (x.data_ptr() | w.data_ptr() | out.data_ptr()) % 16
      or any(np_dtype_of(t) != np.float32 for t in (x, w, out) + ((y,) if y is not None else ()))):
    return None
  return n, d, ldx, (y.stride(0) if y is not None and n > 1 else 1), _ws.get(need, x.device)


@_writes('out')
def rowdot_colsum(x, w, y, out, accumulate=False):
  """out[c] (+)= sum_i x[i, c] * (x[i, :] . w - y[i]) in one pass over the fp32 row tile x [n, d] (y may be None);
  False when the operands do not meet sp_rowdot_colsum_f32's layout (the caller then takes the two-launch form)."""
  ops = _rowdot_operands(x, w, y, out)
  if ops is None:
    return False
  n, d, ldx, ldy, ws = ops
  check(_hip.lib().sp_rowdot_colsum_f32(_p(x), ldx, n, d, _p(w), _p(y), ldy, _p(out), 1 if accumulate else 0, _p(ws),
                                        ws.numel(), _stream()))
  return True


@_writes('out')
def rowdot_link_colsum(x, w, y, out, link, accumulate=False):
  """out[c] (+)= sum_i x[i, c] * (link(x[i, :] . w) - y[i]) in one pass over the fp32 row tile x [n, d] (y may be None),
  link one of _hip.SP_LINK_*: sp_rowdot_link_colsum_f32.  False when the operands do not meet the kernel's layout
  (the caller then takes the launches the expression states); a link the library does not know is an error."""
  ops = _rowdot_operands(x, w, y, out)
  if ops is None:
    return False
  n, d, ldx, ldy, ws = ops
  check(_hip.lib().sp_rowdot_link_colsum_f32(_p(x), ldx, n, d, _p(w), _p(y), ldy, int(link), _p(out),
                                             1 if accumulate else 0, _p(ws), ws.numel(), _stream()))
  return True


gemm = gemm_f32   # dtype-dispatching: fp32 -> sp_gemm_f32, fp64 -> sp_gemm_f64


def _ld(t):
  """Row stride (elements) of a 2-D tensor whose inner stride is 1."""
  assert t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1), (t.shape, t.stride())
  return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def prepare_points(points):
  """What the split tier of nearest_center reads of fp32 points -- two bf16 images and |x|^2 per point -- as a
  buffer to hand to nearest_center(prepared=...) for as long as the points are not written (one k-means fit)."""
  _require_device(points)
  n, d = points.shape
  assert np_dtype_of(points) == np.float32
  lib = _hip.lib()
  out = devarray.empty((max(int(lib.sp_kmeans_points_prepared_bytes(n, d)), 1),), np.uint8)
  check(lib.sp_kmeans_points_prepare(C.c_void_p(points.data_ptr()), _ld(points), n, d, C.c_void_p(out.data_ptr()),
                                     out.numel(), _stream()))
  return out


@_writes('labels')
def nearest_center(points, centers, labels, tier=_hip.NEAREST_AUTO, prepared=None):
  """labels[i] = argmin_c |points[i] - centers[c]| (cdist + argmin; k_means_.py:61-66)."""
  _require_device(points, centers, labels)
  n, d = points.shape
  k, d2 = centers.shape
  assert d == d2 and np_dtype_of(labels) == np.int64 and labels.numel() == n and labels.is_contiguous()
  lib = _hip.lib()
  if prepared is not None:
    ws = _ws.get(lib.sp_nearest_center_prepared_workspace_bytes(n, k, d), points.device)
    check(lib.sp_nearest_center_prepared(C.c_void_p(points.data_ptr()), _hip.sp_dtype(np_dtype_of(points)), _ld(points),
                                         C.c_void_p(prepared.data_ptr()),
                                         C.c_void_p(centers.data_ptr()), _hip.sp_dtype(np_dtype_of(centers)), _ld(centers),
                                         n, k, d, C.c_void_p(labels.data_ptr()), tier, C.c_void_p(ws.data_ptr()),
                                         ws.numel(), _stream()))
    return labels
  need = lib.sp_nearest_center_workspace_bytes(n, k, d)
  ws = _ws.get(need, points.device)
  check(lib.sp_nearest_center(C.c_void_p(points.data_ptr()), _hip.sp_dtype(np_dtype_of(points)), _ld(points),
                              C.c_void_p(centers.data_ptr()), _hip.sp_dtype(np_dtype_of(centers)), _ld(centers),
                              n, k, d, C.c_void_p(labels.data_ptr()), tier, C.c_void_p(ws.data_ptr()),
                              ws.numel(), _stream()))
  return labels


@_writes('counts')
def bincount(labels, k, counts):
  """counts[:k] = np.bincount(labels, minlength=k) (k_means_.py:69-72)."""
  _require_device(labels, counts)
  assert np_dtype_of(labels) == np.int64 and np_dtype_of(counts) == np.int64 and counts.numel() == k
  assert labels.is_contiguous() and counts.is_contiguous()
  check(_hip.lib().sp_bincount_i64(C.c_void_p(labels.data_ptr()), labels.numel(), k,
                                   C.c_void_p(counts.data_ptr()), _stream()))
  return counts


@_writes('out', 'counts')
def segment_sum(points, labels, k, out, counts=None):
  """out[c] = points[labels == c].sum(axis=0) (k_means_.py:75-97); counts (int64 [k], optional) = np.bincount(labels,
  minlength=k): the counting sort inside has the number anyway."""
  _require_device(points, labels, out, counts)
  n, d = points.shape
  assert np_dtype_of(labels) == np.int64 and labels.numel() == n and labels.is_contiguous()
  assert np_dtype_of(out) == np_dtype_of(points) and tuple(out.shape) == (k, d) and out.is_contiguous()
  lib = _hip.lib()
  need = lib.sp_segment_sum_workspace_bytes(n, k, d)
  ws = _ws.get(need, points.device)
  if counts is not None:
    assert np_dtype_of(counts) == np.int64 and counts.numel() == k and counts.is_contiguous()
  check(lib.sp_segment_sum_counts(C.c_void_p(points.data_ptr()), _hip.sp_dtype(np_dtype_of(points)), _ld(points),
                                  C.c_void_p(labels.data_ptr()), n, k, d, C.c_void_p(out.data_ptr()),
                                  C.c_void_p(counts.data_ptr() if counts is not None else 0),
                                  C.c_void_p(ws.data_ptr()), ws.numel(), _stream()))
  return out


RANDOM_KINDS = {'uniform': 0, 'normal': 1, 'randint': 2}


@_writes('out')
def random_fill(out, kind, seed, offset, lo=0, hi=1):
  """Philox fill of a dense tensor: element i = f(seed, offset + i) (srandom.py:38-55)."""
  _require_device(out)
  assert out.is_contiguous()
  check(_hip.lib().sp_random_fill(C.c_void_p(out.data_ptr()), _hip.sp_dtype(np_dtype_of(out)), out.numel(),
                                  RANDOM_KINDS[kind], int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
                                  int(lo), int(hi), _stream()))
  return out


@_writes('out')
def cumscan(src, out, axis, product=False):
  """out = np.cumsum / np.cumprod(src, axis) for dense tensors of one dtype (scan.py:42-63)."""
  _require_device(src, out)
  assert src.is_contiguous() and out.is_contiguous() and np_dtype_of(src) == np_dtype_of(out) and tuple(src.shape) == tuple(out.shape)
  shape = tuple(src.shape)
  outer = int(np.prod(shape[:axis], dtype=np.int64))
  inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
  check(_hip.lib().sp_cumscan(C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()), _hip.sp_dtype(np_dtype_of(src)),
                              outer, shape[axis], inner, 1 if product else 0, _stream()))
  return out


def sort_rows(src, values=True, indices=False):
  """Stable sort of every row of a contiguous [rows, cols] tensor along its last axis (sort.py:68-69, :137-138):
  returns (sorted values or None, int64 argsort or None)."""
  _require_device(src)
  assert src.dim() == 2 and src.is_contiguous()
  rows, cols = src.shape
  vals = devarray.empty((rows, cols), np_dtype_of(src)) if values else None
  idx = devarray.empty((rows, cols), np.int64) if indices else None
  if rows and cols:
    lib = _hip.extras()        # (sort is outside the tile path: libspartan_hip_extras.so)
    dt = _hip.sp_dtype(np_dtype_of(src))
    ws = _ws.get(lib.sp_sort_rows_workspace_bytes(dt, rows, cols), src.device)
    check(lib.sp_sort_rows(C.c_void_p(src.data_ptr()), dt, rows, cols, C.c_void_p(vals.data_ptr() if values else 0),
                           C.c_void_p(idx.data_ptr() if indices else 0), C.c_void_p(ws.data_ptr()), ws.numel(),
                           _stream()))
  return vals, idx


@_writes('a', 'info')
def potrf(a, info):
  """In place: the lower triangle of the square fp32 / fp64 matrix `a` (a view with inner stride 1 will do) becomes
  its Cholesky factor L, the strict upper triangle zero (sp_potrf); `info`, a device int32, receives 0 or the order
  of the first leading minor that is not positive definite.  Nothing waits for the device."""
  _require_device(a, info)
  dt, n = tile_checks.check_potrf(np_dtype_of(a), a.shape)
  assert np_dtype_of(info) == np.int32
  assert n <= 1 or a.stride(1) == 1
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  ws = _ws.get(lib.sp_potrf_workspace_bytes(code, n), a.device)
  check(lib.sp_potrf(code, _p(a), _ld(a), n, _p(ws), ws.numel(), _p(info), _stream()))
  return a


@_writes('b')
def trsm_rlt(b, l):
  """In place: b <- x with x . l^T = b, `l` square lower triangular (its upper triangle is not read), `b` [m, n]; both
  fp32 or both fp64, views with inner stride 1 (sp_trsm_rlt)."""
  _require_device(b, l)
  dt, m, n = tile_checks.check_trsm_rlt(_dtypes(b, l), (b.shape, l.shape))
  assert n <= 1 or (b.stride(1) == 1 and l.stride(1) == 1)
  if m and n:
    check(_hip.extras().sp_trsm_rlt(_hip.sp_dtype(dt), _p(l), _ld(l), n, _p(b), _ld(b), m, _stream()))
  return b


@_writes('w', 'v', 'info')
def syevj(a, w, v, info):
  """Eigenvalues (ascending, into the vector `w`) and eigenvectors (the columns of `v`, same order) of the symmetric
  fp32 / fp64 matrix `a`, whose lower triangle is read and which is NOT written (sp_syevj: cyclic two-sided Jacobi);
  `a` and `v` may be views with inner stride 1.  `info`, a device int32, receives 0, or 1 if 64 sweeps did not
  converge.  Returns the number of sweeps.  The call waits for the device once per sweep (a word that says whether
  the off-diagonal norm is below n u ||a||_F) and for nothing else."""
  _require_device(a, w, v, info)
  dt, n = tile_checks.check_syev(np_dtype_of(a), a.shape, 'syevj')
  assert np_dtype_of(info) == np.int32
  assert np_dtype_of(w) == dt and np_dtype_of(v) == dt and tuple(w.shape) == (n,) and tuple(v.shape) == (n, n)
  assert n <= 1 or (a.stride(1) == 1 and v.stride(1) == 1 and w.stride(0) == 1)
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  ws = _ws.get(lib.sp_syevj_workspace_bytes(code, n), a.device)
  sweeps = C.c_int32(0)
  check(lib.sp_syevj(code, _p(a), _ld(a), n, _p(w), _p(v), _ld(v), _p(ws), ws.numel(), _p(info), C.byref(sweeps),
                     _stream()))
  return int(sweeps.value)


@_writes('dist2', 'idx')
def knn(q, x, k, dist2, idx, index_offset=0, splits=0):
  """dist2[i], idx[i] <- the k rows of `x` [np, d] nearest to row i of `q` [nq, d] by squared Euclidean distance
  (difference form), ascending by (distance, index); idx = index_offset + row of x, padded with +inf / -1 when np < k
  (sp_knn).  q, x: both fp32 or both fp64, views with inner stride 1; dist2 (their dtype) and idx (int64): contiguous
  [nq, k].  splits: 0 = the library chooses into how many ranges the points are cut, s >= 1 = min(s, np) ranges."""
  _require_device(q, x, dist2, idx)
  dt, nq, n, d, k, splits = tile_checks.check_knn(_dtypes(q, x), (q.shape, x.shape), k, splits)
  assert np_dtype_of(dist2) == dt and np_dtype_of(idx) == np.int64
  assert tuple(dist2.shape) == (nq, k) and tuple(idx.shape) == (nq, k) and dist2.is_contiguous() and idx.is_contiguous()
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  need = lib.sp_knn_workspace_bytes(code, nq, n, d, k, splits)
  ws = _ws.get(need, q.device) if need else None
  check(lib.sp_knn(code, _p(q), _ld(q), nq, _p(x), _ld(x), n, d, k, int(index_offset), splits, _p(dist2), _p(idx),
                   _p(ws), ws.numel() if need else 0, _stream()))
  return dist2, idx


@_writes('dist2', 'idx')
def knn_merge(cand_dist2, cand_idx, k, dist2, idx):
  """dist2[i], idx[i] <- the k smallest by (distance, index) of the m candidates of row i; candidates with a negative
  index are padding (sp_knn_merge).  cand_dist2 (fp32 / fp64) and cand_idx (int64): [nq, m] views with inner stride 1
  and ONE row stride; dist2, idx: contiguous [nq, k]."""
  _require_device(cand_dist2, cand_idx, dist2, idx)
  dt, nq, m, k = tile_checks.check_knn_merge(_dtypes(cand_dist2, cand_idx), (cand_dist2.shape, cand_idx.shape), k)
  assert np_dtype_of(idx) == np.int64 and np_dtype_of(dist2) == dt
  assert _ld(cand_dist2) == _ld(cand_idx), (cand_dist2.stride(), cand_idx.stride())
  assert tuple(dist2.shape) == (nq, k) and tuple(idx.shape) == (nq, k) and dist2.is_contiguous() and idx.is_contiguous()
  check(_hip.extras().sp_knn_merge(_hip.sp_dtype(dt), _p(cand_dist2), _p(cand_idx), _ld(cand_dist2), nq, m, k, _p(dist2),
                                   _p(idx), _stream()))
  return dist2, idx


@_writes('sim', 'idx')
def item_topk(targets, tnorm, sources, snorm, k, sim, idx, index_offset=0, splits=0):
  """sim[j], idx[j] <- the k columns of `sources` [users, ns] of the largest cosine similarity with column j of
  `targets` [users, m], by (similarity descending, index ascending); idx = index_offset + column of sources, padded
  with -inf / -1 when ns < k (sp_item_topk; include/spartan_hip_cf.h states the arithmetic: dot over the users in
  ascending order, / (tnorm[j] * snorm[i]), nan_to_num).  targets, sources: both fp32 or both fp64, views with inner
  stride 1 (two column ranges of one table will do); tnorm [m], snorm [ns] contiguous, of their dtype; sim (their
  dtype) and idx (int64): contiguous [m, k].  splits: 0 = the library chooses into how many ranges the sources are cut,
  s >= 1 = min(s, ns) ranges.  Refusals: tile_checks.check_item_topk_operands', before any launch.  Owns the workspace.
  Returns the number of kernels the library issues: 1, or 2 where it needs a workspace (more than one range, whose
  candidates the second kernel merges)."""
  _require_device(targets, tnorm, sources, snorm, sim, idx)
  dt, users, m, ns, k, splits = tile_checks.check_item_topk_operands(
      _dtypes(targets, tnorm, sources, snorm, sim), targets.shape, tnorm.shape, sources.shape,
      snorm.shape, k, splits)
  assert np_dtype_of(idx) == np.int64 and tnorm.is_contiguous() and snorm.is_contiguous()
  assert tuple(sim.shape) == (m, k) and tuple(idx.shape) == (m, k) and sim.is_contiguous() and idx.is_contiguous()
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  need = lib.sp_item_topk_workspace_bytes(code, users, m, ns, k, splits)
  ws = _ws.get(need, targets.device) if need else None
  check(lib.sp_item_topk(code, _p(targets), _ld(targets), _p(tnorm), m, _p(sources), _ld(sources), _p(snorm), ns, users,
                         k, int(index_offset), splits, _p(sim), _p(idx), _p(ws), ws.numel() if need else 0, _stream()))
  return 2 if need else 1


@_writes('sim', 'idx')
def item_topk_merge(cand_sim, cand_idx, k, sim, idx):
  """sim[j], idx[j] <- the k best by (similarity descending, index ascending) of the candidates of row j; candidates
  with a negative index are padding (sp_item_topk_merge).  cand_sim (fp32 / fp64) and cand_idx (int64): [m, cands]
  views with inner stride 1 and ONE row stride; sim, idx: contiguous [m, k]."""
  _require_device(cand_sim, cand_idx, sim, idx)
  dt, m, cands, k = tile_checks.check_item_topk_merge(_dtypes(cand_sim, cand_idx), (cand_sim.shape, cand_idx.shape), k)
  assert np_dtype_of(idx) == np.int64 and np_dtype_of(sim) == dt
  assert _ld(cand_sim) == _ld(cand_idx), (cand_sim.stride(), cand_idx.stride())
  assert tuple(sim.shape) == (m, k) and tuple(idx.shape) == (m, k) and sim.is_contiguous() and idx.is_contiguous()
  check(_hip.extras().sp_item_topk_merge(_hip.sp_dtype(dt), _p(cand_sim), _p(cand_idx), _ld(cand_sim), m, cands, k,
                                         _p(sim), _p(idx), _stream()))
  return sim, idx


@_writes('d', 'info')
def apsp(d, info):
  """In place: the square fp32 / fp64 matrix `d` of edge lengths (>= 0, +inf = no edge, the diagonal taken as 0; a view
  with inner stride 1 will do) becomes the matrix of shortest-path lengths, +inf where there is no path (sp_apsp:
  blocked Floyd-Warshall, a candidate d[i][k] + d[k][j] wins only if it is smaller).  `info`, a device int32, receives
  0, or 1 if an off-diagonal entry is NaN or negative (`d` is then unspecified).  Nothing waits for the device."""
  _require_device(d, info)
  dt, n = tile_checks.check_apsp(np_dtype_of(d), d.shape)
  assert np_dtype_of(info) == np.int32
  assert n <= 1 or d.stride(1) == 1
  check(_hip.extras().sp_apsp(_hip.sp_dtype(dt), _p(d), _ld(d), n, _p(info), _stream()))
  return d


@_writes('w')
def graph_from_knn(dist, idx, w):
  """w [n, n] <- the dense undirected graph of the neighbour lists dist (fp32 / fp64, >= 0) and idx (int64), both [n, k]
  views with inner stride 1 and ONE row stride: +inf, 0 on the diagonal, and for every listed pair (i, idx[i][e]) the
  smallest weight stated for it in either direction, on both sides; idx < 0 is padding (sp_graph_from_knn).  `w`: of
  dist's dtype, a view with inner stride 1."""
  _require_device(dist, idx, w)
  dt, n, k = tile_checks.check_graph_from_knn(_dtypes(dist, idx), (dist.shape, idx.shape))
  assert np_dtype_of(w) == dt
  assert tuple(w.shape) == (n, n) and (n <= 1 or w.stride(1) == 1)
  assert k <= 1 or (dist.stride(1) == 1 and idx.stride(1) == 1)
  assert n <= 1 or _ld(dist) == _ld(idx), (dist.stride(), idx.stride())
  check(_hip.extras().sp_graph_from_knn(_hip.sp_dtype(dt), _p(dist), _p(idx), _ld(dist), n, k, _p(w), _ld(w), _stream()))
  return w


@_writes('x', 'info')
def als_solve(r, y, la, alpha, implicit, x, info):
  """x[i] <- the solution of row i's normal equations of one ALS half-step: ratings `r` [m, n], factors `y` [n, f],
  both fp32 or both fp64, views with inner stride 1; `x` [m, f] of their dtype, a view with inner stride 1
  (sp_als_solve; include/spartan_hip_als.h states the two modes).  `info`, a device int32 the caller has zeroed,
  receives 1 + the lowest row whose system is not positive definite if it is still 0; that row of x is NaN.  TypeError
  for other dtypes, ValueError for shapes that do not fit or f outside 1 .. 64.  Nothing waits for the device."""
  _require_device(r, y, x, info)
  dt, m, n, f = tile_checks.check_als_solve(_dtypes(r, y), (r.shape, y.shape))
  if tuple(x.shape) != (m, f) or np_dtype_of(x) != dt:
    raise ValueError('als_solve: a target of shape %s and dtype %s for %d rows and %d features of %s'
                     % (tuple(x.shape), np_dtype_of(x), m, f, dt))
  assert np_dtype_of(info) == np.int32
  if m == 0:
    return x
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  ws = _ws.get(lib.sp_als_solve_workspace_bytes(code, m, n, f, int(bool(implicit))), r.device)
  check(lib.sp_als_solve(code, _p(r), _ld(r), m, n, _p(y), _ld(y), f, float(la), float(alpha), int(bool(implicit)), _p(x),
                         _ld(x), _p(info), _p(ws), ws.numel(), _stream()))
  return x


@_writes('labels', 'sums', 'wsum', 'u')
def fuzzy_step(points, centers, m, labels, sums, wsum, u=None, splits=0):
  """One iteration of the reference's fuzzy k-means on a row tile (sp_fuzzy_step; include/spartan_hip_fuzzy.h states
  the arithmetic and its order): `points` [n, d] and `centers` [k, d], both fp32 or both fp64, views with inner stride
  1; labels [n] int64 contiguous (or None) <- the lowest centre at the largest distance, sums [k, d] (a view with inner
  stride 1) <- sum_i w_ij x_i, wsum [k] contiguous <- sum_i w_ij, and, only if `u` [n, k] (a view with inner stride 1)
  is passed, u <- the memberships.  splits: 0 = the library chooses into how many ranges the rows are cut, s >= 1 =
  min(s, ceil(n / 64)) ranges.  TypeError for other or mixed dtypes, ValueError for m that is not finite and > 1,
  k < 1 or shapes that do not fit -- all before any launch.  Nothing waits for the device."""
  _require_device(points, centers, labels, sums, wsum, u)
  dt, n, k, d, m, splits = tile_checks.check_fuzzy_step(_dtypes(points, centers, sums, wsum, u),
                                                        (points.shape, centers.shape), m, splits)
  if tuple(sums.shape) != (k, d) or tuple(wsum.shape) != (k,) or (u is not None and tuple(u.shape) != (n, k)):
    raise ValueError('fuzzy_step: targets of shapes %s, %s, %s for %d rows, %d centres and %d features'
                     % (tuple(sums.shape), tuple(wsum.shape), None if u is None else tuple(u.shape), n, k, d))
  if labels is not None and (tuple(labels.shape) != (n,) or np_dtype_of(labels) != np.int64):
    raise ValueError('fuzzy_step: labels of shape %s and dtype %s for %d rows' % (tuple(labels.shape), np_dtype_of(labels), n))
  assert wsum.is_contiguous() and (labels is None or labels.is_contiguous())
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  ws = _ws.get(lib.sp_fuzzy_step_workspace_bytes(code, n, k, d, splits), points.device)
  check(lib.sp_fuzzy_step(code, _p(points), _ld(points), n, _p(centers), _ld(centers), k, d, m, splits, _p(labels),
                          _p(sums), _ld(sums), _p(wsum), _p(u), k if u is None else _ld(u), _p(ws), ws.numel(), _stream()))
  return labels, sums, wsum, u


@_writes('delta', 'doc_topics')
def lda_step(x, n, alpha, eta, iters, delta=None, doc_topics=None, splits=0):
  """One CVB0 step of the reference's LDA on a tile of documents (sp_lda_step; include/spartan_hip_lda.h states the
  arithmetic and its order): `x` [V, D] terms x documents and `n` [k, V] topic / term counts, both fp32 or both fp64,
  views with inner stride 1; delta [k, V] (a view with inner stride 1, or None) <- the sum over the documents of the
  last inner iteration's q, doc_topics [D, k] (the same, or None) <- gamma, NaN rows for empty documents.  splits:
  0 = the library chooses into how many ranges the documents are cut, s >= 1 = min(s, ceil(D / 64)) ranges.  TypeError
  for other or mixed dtypes, ValueError for k outside 1 .. 128, iters < 1, alpha or eta not finite and > 0 or shapes
  that do not fit -- all before any launch.  Nothing waits for the device."""
  _require_device(x, n, delta, doc_topics)
  dt, v, d, k, alpha, eta, iters, splits = tile_checks.check_lda_step(_dtypes(x, n, delta, doc_topics), (x.shape, n.shape),
                                                                      alpha, eta, iters, splits)
  if (delta is not None and tuple(delta.shape) != (k, v)) or (doc_topics is not None and tuple(doc_topics.shape) != (d, k)):
    raise ValueError('lda_step: targets of shapes %s, %s for %d terms, %d documents and %d topics'
                     % (None if delta is None else tuple(delta.shape),
                        None if doc_topics is None else tuple(doc_topics.shape), v, d, k))
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  ws = _ws.get(lib.sp_lda_step_workspace_bytes(code, v, d, k, iters, splits), x.device)
  check(lib.sp_lda_step(code, _p(x), _ld(x), v, d, _p(n), _ld(n), k, alpha, eta, iters, splits, _p(delta),
                        v if delta is None else _ld(delta), _p(doc_topics), k if doc_topics is None else _ld(doc_topics),
                        _p(ws), ws.numel(), _stream()))
  return delta, doc_topics


@_writes('out_s', 'out_df', 'out_bad')
def nb_step(x, labels, label_size, out_s, out_df, out_bad, splits=0):
  """The tile body of the reference's naive Bayes fit on a row tile (sp_nb_step; include/spartan_hip_nb.h states the
  arithmetic and its order): `x` [m, d] fp32 or fp64, a view with inner stride 1; `labels` int64, [m] or an [m, 1]
  view, its elements next to each other.  out_s [label_size, d] of x's dtype (a view with inner stride 1) <- the sum
  over each label's rows of x_i / sqrt(mean_j x_ij^2), out_df [d] int64 contiguous <- the rows with x_ij > 0, out_bad
  [1] int64 <- 0, or 1 + the lowest row whose label is outside 0 .. label_size - 1 (that row is left out of out_s
  and kept in out_df).  splits: 0 = the library chooses into how many ranges the rows are cut, s >= 1 =
  min(s, ceil(m / 64)) ranges.  TypeError for other dtypes, ValueError for label_size outside 1 .. 128 or shapes that
  do not fit -- all before any launch.  Nothing waits for the device."""
  _require_device(x, labels, out_s, out_df, out_bad)
  dt = np_dtype_of(x)
  m, d, label_size = tile_checks.check_nb_operands(dt, x.shape, np_dtype_of(labels), labels.shape, label_size, splits)
  tile_checks.one_float_dtype('nb_step', (dt, np_dtype_of(out_s)))
  if tuple(out_s.shape) != (label_size, d) or tuple(out_df.shape) != (d,) or tuple(out_bad.shape) != (1,):
    raise ValueError('nb_step: targets of shapes %s, %s, %s for %d labels and %d features'
                     % (tuple(out_s.shape), tuple(out_df.shape), tuple(out_bad.shape), label_size, d))
  if np_dtype_of(out_df) != np.int64 or np_dtype_of(out_bad) != np.int64:
    raise TypeError('nb_step: df and bad are int64, got %s and %s' % (np_dtype_of(out_df), np_dtype_of(out_bad)))
  assert m <= 1 or labels.stride(0) == 1, labels.stride()
  assert out_df.is_contiguous()
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  ws = _ws.get(lib.sp_nb_step_workspace_bytes(code, m, d, label_size, int(splits)), x.device)
  check(lib.sp_nb_step(code, _p(x), _ld(x), m, d, _p(labels), label_size, int(splits), _p(out_s), _ld(out_s), _p(out_df),
                       _p(out_bad), _p(ws), ws.numel(), _stream()))
  return out_s, out_df, out_bad


@_writes('ax', 'ay', 'az')
def nbody_accel(x, y, z, mass, r0, m, ax, ay, az, g, rmin, splits=0):
  """The accelerations of bodies r0 .. r0 + m - 1 under the gravity of all n (sp_nbody_accel;
  include/spartan_hip_nbody.h states the arithmetic of a pair and the order of a target's sum): `x`, `y`, `z`, `mass`
  contiguous [n], all fp32 or all fp64; ax, ay, az contiguous [m] of their dtype <- sum over i != j of
  (g mass_i) / max(r_ij, rmin)^3 * (x_i - x_j) (y, z alike).  Nothing of size n x n is stored.  splits: 0 = the
  library chooses from n into how many ranges the sources are cut, s >= 1 = min(s, ceil(n / 64)) ranges.  TypeError for
  other or mixed dtypes, ValueError for shapes that do not fit, targets that are not among the bodies, splits < 0, a g
  that is not finite or an rmin that is not finite and > 0 -- all before any launch.  Owns the workspace.  Nothing
  waits for the device.  Returns the number of kernels the library issues: 1, or 2 where it needs a workspace (more than
  one range, whose partial sums the second kernel adds)."""
  _require_device(x, y, z, mass, ax, ay, az)
  operands = (x, y, z, mass, ax, ay, az)
  dt, n, r0, m, g, rmin, splits = tile_checks.check_nbody_operands(_dtypes(*operands), [t.shape for t in operands[:4]],
                                                                   r0, m, g, rmin, splits)
  if any(tuple(t.shape) != (m,) for t in (ax, ay, az)):
    raise ValueError('nbody_accel: targets of shapes %s for %d bodies' % ([tuple(t.shape) for t in (ax, ay, az)], m))
  assert all(t.is_contiguous() for t in operands), [t.stride() for t in operands]
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  need = lib.sp_nbody_accel_workspace_bytes(code, n, m, splits)
  ws = _ws.get(need, x.device) if need else None
  check(lib.sp_nbody_accel(code, g, rmin, _p(x), _p(y), _p(z), _p(mass), n, r0, m, _p(ax), _p(ay), _p(az), splits, _p(ws),
                           ws.numel() if need else 0, _stream()))
  return 2 if need else 1


def _side_by_side(t, n):
  """Whether the n elements of `t` -- [n] or an [n, 1] view -- lie next to each other in memory."""
  return int(t.numel()) == n and (n <= 1 or t.stride(0) == 1)


@_writes('alpha_out', 'w_out')
def svm_dca(x, y, alpha, w0, scaled_lambda, chains, alpha_out, w_out=None):
  """One pass of the reference's dual coordinate ascent over the rows of a tile (sp_svm_dca;
  include/spartan_hip_svm.h states the arithmetic of a row and the order of its two inner products): `x` [m, d] fp32 or
  fp64, a view with inner stride 1; `y`, `alpha` ([m] or [m, 1]) and `w0` ([d] or [d, 1]) of its dtype, each with its
  elements next to each other.  The rows are cut into `chains` consecutive bands; every band starts from w = w0 and
  walks its rows in order.  alpha_out ([m] or [m, 1], elements next to each other; it may be `alpha` itself) <- the
  new dual variables, w_out ([chains, d] contiguous, or None) <- the w every chain ends with.  TypeError for other or
  mixed dtypes, ValueError for d outside 1 .. 4096, chains < 1, a scaled_lambda that is not finite and > 0 or shapes
  that do not fit -- all before any launch.  One kernel, no workspace.  Nothing waits for the device."""
  _require_device(x, y, alpha, w0, alpha_out, w_out)
  dt, m, d, scaled_lambda, chains = tile_checks.check_svm_dca(
      _dtypes(x, y, alpha, w0, alpha_out, w_out)[:4], (x.shape, y.shape, alpha.shape, w0.shape), scaled_lambda, chains)
  tile_checks.one_float_dtype('svm_dca', _dtypes(x, alpha_out, w_out))
  if tuple(alpha_out.shape) not in ((m,), (m, 1)) or (w_out is not None and tuple(w_out.shape) != (chains, d)):
    raise ValueError('svm_dca: targets of shapes %s, %s for %d rows, %d chains and %d features'
                     % (tuple(alpha_out.shape), None if w_out is None else tuple(w_out.shape), m, chains, d))
  assert all(_side_by_side(t, m) for t in (y, alpha, alpha_out)) and _side_by_side(w0, d), \
      [t.stride() for t in (y, alpha, alpha_out, w0)]
  assert w_out is None or w_out.is_contiguous()
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  check(lib.sp_svm_dca(_hip.sp_dtype(dt), _p(x), _ld(x), m, d, _p(y), _p(alpha), _p(w0), scaled_lambda, chains,
                       _p(alpha_out), _p(w_out), _stream()))
  return alpha_out, w_out


@_writes('out')
def lmm_swaption(eps, maturities, lamb, delta, f0, theta, out):
  """out[p] <- the discounted payoff of one swaption under the LIBOR market model, the mean over the antithetic pair p
  of paths (sp_lmm_swaption; include/spartan_hip_lmm.h states the recurrence, operation for operation): `eps` [S, n]
  fp32 or fp64 draws, a view with inner stride 1 (a band of columns of a wider array is taken as it is); `out` [n] of
  its dtype, contiguous.  TypeError for other or mixed dtypes, ValueError for S and K = `maturities` that do not satisfy
  1 <= S < K <= SP_LMM_MAX_K, scalars that are not finite, delta <= 0 or a target that does not fit -- all before any
  launch.  One kernel (none for n = 0), no workspace.  Nothing waits for the device."""
  _require_device(eps, out)
  dt, n, s, k, lamb, delta, f0, theta = tile_checks.check_lmm_swaption(np_dtype_of(eps), eps.shape, maturities, lamb,
                                                                       delta, f0, theta)
  tile_checks.one_float_dtype('lmm_swaption', _dtypes(eps, out))
  if tuple(out.shape) != (n,):
    raise ValueError('lmm_swaption: a target of shape %s for %d pairs' % (tuple(out.shape), n))
  assert out.is_contiguous()
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  check(lib.sp_lmm_swaption(_hip.sp_dtype(dt), _p(eps), _ld(eps), n, s, k, lamb, delta, f0, theta, _p(out), _stream()))
  return out


@_writes('centers', 'counts', 'rows', 'num')
def canopy(x, t1, t2, chains, cap, centers, counts, rows, num):
  """The greedy canopy pass of the reference over the rows of a tile (sp_canopy; include/spartan_hip_canopy.h states
  the arithmetic and the order of a canopy's sum): `x` [n, d] fp32 or fp64, a view with inner stride 1, cut into
  `chains` consecutive bands.  Chain c writes its canopies in creation order to the slots c * cap .. of `centers`
  [chains * cap, d] of x's dtype (the means; a view with inner stride 1), `counts` and `rows` [chains * cap] int64
  contiguous (the observed rows; the creating row's index in x), and their number -- or -1 where `cap` does not suffice
  -- to `num` [chains] int64.  TypeError for other or mixed dtypes, ValueError for d < 1, chains < 1, cap < 1,
  thresholds that are not finite or targets that do not fit -- all before any launch.  One kernel; owns the workspace.
  Nothing waits for the device."""
  _require_device(x, centers, counts, rows, num)
  dt, n, d, t1, t2, chains, cap, _ = tile_checks.check_canopy(np_dtype_of(x), x.shape, t1, t2, chains, cap)
  tile_checks.one_float_dtype('canopy', _dtypes(x, centers))
  slots = chains * cap
  if tuple(centers.shape) != (slots, d) or any(tuple(t.shape) != s for t, s in ((counts, (slots,)), (rows, (slots,)),
                                                                               (num, (chains,)))):
    raise ValueError('canopy: targets of shapes %s for %d chains of at most %d canopies and %d features'
                     % ([tuple(t.shape) for t in (centers, counts, rows, num)], chains, cap, d))
  if any(np_dtype_of(t) != np.int64 for t in (counts, rows, num)):
    raise TypeError('canopy: counts, rows and num are int64, got %s' % ([np_dtype_of(t) for t in (counts, rows, num)],))
  assert all(t.is_contiguous() for t in (counts, rows, num))
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  ws = _ws.get(lib.sp_canopy_workspace_bytes(code, n, d, chains, cap), x.device)
  check(lib.sp_canopy(code, _p(x), _ld(x), n, d, t1, t2, chains, cap, _p(centers), _ld(centers), _p(counts), _p(rows),
                      _p(num), _p(ws), ws.numel(), _stream()))
  return centers, counts, rows, num


@_writes('labels')
def pdf_label(x, centers, labels):
  """labels[i] <- the lowest j at which 1 / (1 + |x_i - c_j|^2) is largest, -1 where there is none (sp_pdf_label;
  include/spartan_hip_canopy.h says why this is not an arg-min of the distance): `x` [n, d] and `centers` [k, d] fp32
  or fp64 alike, views with inner stride 1; `labels` [n] int32 contiguous.  TypeError for other or mixed dtypes and a
  target that is not int32, ValueError for shapes that do not fit -- all before any launch.  One kernel (none for
  n = 0), no workspace.  Nothing waits for the device."""
  _require_device(x, centers, labels)
  dt, n, k, d = tile_checks.check_pdf_label(_dtypes(x, centers), (x.shape, centers.shape))
  if tuple(labels.shape) != (n,):
    raise ValueError('pdf_label: a target of shape %s for %d rows' % (tuple(labels.shape), n))
  if np_dtype_of(labels) != np.int32:
    raise TypeError('pdf_label: labels are int32, got %s' % (np_dtype_of(labels),))
  assert labels.is_contiguous()
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  check(lib.sp_pdf_label(_hip.sp_dtype(dt), _p(x), _ld(x), n, _p(centers) if k else None, _ld(centers), k, d, _p(labels),
                         _stream()))
  return labels


def sgd_mf_plan(m, n, indptr, indices):
  """The level schedule of a tile of ratings [m, n] in canonical CSR (sp_sgd_mf_plan; include/spartan_hip_mf.h states
  its layout) from HOST arrays `indptr` [m + 1] and `indices` [nnz]: a uint8 array of the bytes in use.  Host code: no
  device is needed.  HipError for what the library refuses (nnz >= 2^31, an indptr that is not monotone from 0 to nnz, an
  index outside 0 .. n - 1)."""
  indptr = np.ascontiguousarray(indptr, dtype=np.int64)
  indices = np.ascontiguousarray(indices, dtype=np.int32)
  m, n, nnz = int(m), int(n), int(indices.shape[0])
  if indptr.shape != (m + 1,):
    raise ValueError('sgd_mf_plan: indptr of shape %s for %d rows' % (indptr.shape, m))
  lib = _hip.extras()
  need = int(lib.sp_sgd_mf_plan_bytes(m, n, nnz))
  if need == 0:
    raise _hip.HipError('sp_sgd_mf_plan: bad sizes m=%d n=%d nnz=%d (each below 2^31)' % (m, n, nnz))
  buf = np.empty((need + 7) // 8, np.int64)               # (8-byte aligned)
  check(lib.sp_sgd_mf_plan(m, n, nnz, indptr.ctypes.data, indices.ctypes.data if nnz else None, buf.ctypes.data, need))
  return buf.view(np.uint8)[:int(buf[6])].copy()


def sgd_mf_plan_parts(plan):
  """The arrays of a plan (a uint8 host array as sgd_mf_plan returns it) as views: {'m', 'n', 'nnz', 'levels', 'wide',
  'entry', 'row', 'col' [nnz], 'level_off' [levels + 1], 'segments' [segments, 4] of (kind, first level, last level + 1,
  0); kind 1 is a wide level, 0 a run of narrow ones}."""
  head = plan[:128].view(np.int64)
  m, n, nnz, levels, segs = (int(v) for v in head[1:6])
  i32 = lambda off, count: plan[int(off):int(off) + 4 * count].view(np.int32)   # noqa: E731
  return {'m': m, 'n': n, 'nnz': nnz, 'levels': levels, 'wide': int(head[12]), 'entry': i32(head[7], nnz),
          'row': i32(head[8], nnz), 'col': i32(head[9], nnz), 'level_off': i32(head[10], levels + 1),
          'segments': i32(head[11], 4 * segs).reshape(segs, 4)}


def sgd_mf_host(shape, indptr, indices, vals, u, m, lr=None, abs_err=None, order=None):
  """The SGD sequence of include/spartan_hip_mf.h as the library's plain host loop (sp_sgd_mf_host) on NumPy arrays:
  the tile `shape` with `indptr`, `indices`, `vals`; `u` [rows, f] and `m` [cols, f] (C-contiguous rows, of vals' dtype)
  are updated IN PLACE; `abs_err` [nnz] (or None) <- |d| per entry; `order` (int32 [nnz], or None for tile order) is the
  order in which the entries are taken.  Refusals: tile_checks.check_sgd_mf's, then the library's."""
  dt, rows, cols, f, lr = tile_checks.check_sgd_mf([vals.dtype, u.dtype, m.dtype], shape, u.shape, m.shape, lr)
  indptr = np.ascontiguousarray(indptr, dtype=np.int64)
  indices = np.ascontiguousarray(indices, dtype=np.int32)
  vals = np.ascontiguousarray(vals)
  nnz = int(indices.shape[0])
  assert indptr.shape == (rows + 1,) and vals.shape == (nnz,), (indptr.shape, vals.shape)
  for t in (u, m):
    assert t.strides[1] == t.itemsize and t.strides[0] % t.itemsize == 0 and t.flags.writeable, t.strides
  if abs_err is not None:
    assert abs_err.dtype == dt and abs_err.shape == (nnz,) and abs_err.flags.c_contiguous
  if order is not None:
    order = np.ascontiguousarray(order, dtype=np.int32)
    assert order.shape == (nnz,)
  ld = lambda t: max(t.strides[0] // t.itemsize, f) if t.shape[0] > 1 else f   # noqa: E731
  ptr = lambda t: None if t is None or t.size == 0 else t.ctypes.data          # noqa: E731
  check(_hip.extras().sp_sgd_mf_host(_hip.sp_dtype(dt), rows, cols, f, nnz, indptr.ctypes.data, ptr(indices), ptr(vals),
                                     ptr(u), ld(u), ptr(m), ld(m), lr, ptr(abs_err), ptr(order)))


@_writes('u', 'm', 'abs_err')
def sgd_mf(shape, vals, plan_dev, plan_host, u, m, lr=None, abs_err=None):
  """One SGD pass over a tile of ratings of `shape` whose values are `vals` [nnz] (sp_sgd_mf; include/spartan_hip_mf.h
  states the sequence and the order of its dot): `u` [rows, f] and `m` [cols, f], fp32 or fp64 like `vals`, views with
  inner stride 1, are updated IN PLACE with the bits of the sequential loop; `plan_host` is sgd_mf_plan's array for
  the tile's structure and `plan_dev` its copy in HBM; `abs_err` ([nnz] contiguous, or None) <- |d| per entry.  Returns
  the number of kernels launched (one per segment of the plan; 0 for an empty tile).  TypeError for other or mixed
  dtypes, ValueError for shapes that do not fit, f outside 1 .. 512 and an lr that is not finite -- all before any
  launch.  Nothing waits for the device."""
  _require_device(vals, plan_dev, u, m, abs_err)
  dt, rows, cols, f, lr = tile_checks.check_sgd_mf(_dtypes(vals, u, m), shape, u.shape, m.shape, lr)
  nnz = int(vals.numel())
  if abs_err is not None:
    tile_checks.one_float_dtype('sgd_mf', _dtypes(vals, abs_err))
    if tuple(abs_err.shape) != (nnz,):
      raise ValueError('sgd_mf: abs_err of shape %s for %d ratings' % (tuple(abs_err.shape), nnz))
    assert abs_err.is_contiguous()
  assert nnz <= 1 or vals.stride(0) == 1
  if nnz == 0:
    return 0
  launched = C.c_int64(0)
  check(_hip.extras().sp_sgd_mf(_hip.sp_dtype(dt), rows, cols, f, nnz, _p(vals), _p(plan_dev), plan_host.ctypes.data, _p(u),
                                _ld(u), _p(m), _ld(m), lr, _p(abs_err), C.byref(launched), _stream()))
  return int(launched.value)


@_writes('deg')
def affinity_degree(x, y, metric, gamma, deg):
  """deg[i] <- sum_j a(x_i, y_j) over all rows of `y` (sp_affinity_degree; include/spartan_hip_spectral.h states the
  measures and the order of the sum): `x` [m, d] and `y` [n, d], both fp32 or both fp64, views with inner stride 1;
  deg [m] contiguous, of their dtype.  metric: 'rbf' (exp(-gamma d2)), 'euclidean', 'manhattan'.  Nothing of size m x n
  is stored.  TypeError for other or mixed dtypes, ValueError for an unknown metric, a gamma that is not finite or
  shapes that do not fit, NotImplementedError for 'scaled_euclidean' -- all before any launch.  Nothing waits for the
  device."""
  _require_device(x, y, deg)
  dt, m, n, d, code_m, gamma = tile_checks.check_affinity_degree(_dtypes(x, y, deg), (x.shape, y.shape), metric, gamma)
  if tuple(deg.shape) != (m,):
    raise ValueError('affinity_degree: a target of shape %s for %d rows' % (tuple(deg.shape), m))
  assert deg.is_contiguous()
  lib = _hip.extras()        # (outside the tile path: libspartan_hip_extras.so)
  code = _hip.sp_dtype(dt)
  need = lib.sp_affinity_degree_workspace_bytes(code, m, n, d)
  ws = _ws.get(need, x.device) if need else None
  check(lib.sp_affinity_degree(code, code_m, gamma, _p(x), _ld(x), m, _p(y), _ld(y), n, d, _p(deg), _p(ws),
                               ws.numel() if need else 0, _stream()))
  return deg


@_writes('out')
def affinity_matrix(x, r0, y, metric, gamma, out, scale=None):
  """out[i, j] <- a(x_i, y_j), where row i of `x` [m, d] is point r0 + i of the n points `y` [n, d]; with `scale` [n]
  (contiguous): a_ij * (scale[r0 + i] * scale[j]) and exactly 1 at j = r0 + i (sp_affinity_matrix;
  include/spartan_hip_spectral.h).  Operands all fp32 or all fp64, views with inner stride 1; out [m, n] the same.
  Refusals as affinity_degree's, and ValueError for r0 < 0 or r0 + m > n.  Nothing waits for the device."""
  _require_device(x, y, out, scale)
  dt, m, n, d, code_m, gamma, r0 = tile_checks.check_affinity_matrix(
      _dtypes(x, y, scale, out), [t.shape for t in (x, y, scale) if t is not None], r0, metric, gamma)
  if tuple(out.shape) != (m, n):
    raise ValueError('affinity_matrix: a target of shape %s for %d rows and %d points' % (tuple(out.shape), m, n))
  assert (n <= 1 or out.stride(1) == 1) and (scale is None or scale.is_contiguous())
  check(_hip.extras().sp_affinity_matrix(_hip.sp_dtype(dt), code_m, gamma, _p(x), _ld(x), m, r0, _p(y), _ld(y), n, d,
                                         _p(scale), _p(out), _ld(out), _stream()))
  return out


def gather_rows(src, idx):
  """src[idx] along axis 0 for a contiguous tensor and a device int64 index vector (filter.py:50-75)."""
  _require_device(src, idx)
  assert src.is_contiguous() and np_dtype_of(idx) == np.int64 and idx.is_contiguous()
  n = int(idx.numel())
  row = int(np.prod(src.shape[1:], dtype=np.int64)) * _elsize(src)
  out = devarray.empty((n,) + tuple(src.shape[1:]), np_dtype_of(src))
  check(_hip.lib().sp_gather_rows(C.c_void_p(src.data_ptr()), row, int(src.shape[0]), C.c_void_p(idx.data_ptr()), n, row,
                                  C.c_void_p(out.data_ptr()), _stream()))
  return out


@_writes('dst')
def stream_copy(dst, src, nbytes=None, max_workgroups=0, stream=None):
  """dst <- src (contiguous bytes); max_workgroups > 0 bounds the grid (a transfer that takes a limited share of
  the CUs, see sp_stream_copy_wg)."""
  _require_device(dst, src)
  n = src.numel() * _elsize(src) if nbytes is None else int(nbytes)
  check(_hip.lib().sp_stream_copy_wg(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), n, int(max_workgroups),
                                     (stream or devarray.current_stream()).ptr))
  return dst
