"""Inputs, references and error bounds for sp_cumscan (csrc/update.hip) and the scan operator (expr/scan.py).
Pure NumPy.

A tile is viewed as [outer, A, inner] and scanned along A.  inner > 1 runs the column kernel (one thread per line, in
NumPy's sequential order: bit equality with np.cumsum / np.cumprod of the same dtype).  inner == 1 runs the row kernel
(64 elements per step by a shuffle scan, a carry between steps): another summation order, so floats are compared with
a reference accumulated in a wider type under a derived bound.

Bounds (derived, not measured).  eps = 2^-23 or 2^-52 (numpy.finfo.eps, twice the unit roundoff u).
  sum      Element j (counted from 0) is a sum of j + 1 terms.  Whatever the order, every term passes through at most j
           additions, each of relative error <= u, so |got_j - ref_j| <= ((1 + u)^j - 1) sum_{i<=j} |x_i|
           <= j eps cumsum(|x|)_j for j u < 1 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).
  product  j multiplications of relative error <= u each: |got_j / ref_j - 1| <= (1 + u)^j - 1 <= j eps, as long as
           nothing under- or overflows (the product lines keep every prefix within 2^+-40).
Integers are exact: np.cumsum / np.cumprod with dtype = the input's wrap modulo 2^32 / 2^64, and so must the kernel.
"""
import functools

import numpy as np

LD = np.longdouble
DTYPES = (np.float32, np.float64, np.int32, np.int64)
FLOATS = (np.float32, np.float64)
EPS = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}
WIDER = {np.dtype(np.float32): np.float64, np.dtype(np.float64): LD}
EXACT_BELOW = {np.dtype(np.float32): 2 ** 24, np.dtype(np.float64): 2 ** 53}

# row kernel: the chunk is 64 lanes; 4 lines per block
ROW_A = (1, 2, 63, 64, 65, 127, 128, 129, 1000)
ROW_OUTER = (1, 3, 4, 5)
ROW_SHAPES = tuple((o, a, 1) for a in ROW_A for o in ROW_OUTER)
ROW_STRIDE_SHAPE = (16384 + 5, 70, 1)        # more lines than the grid has waves: the line loop strides
# column kernel: 256 threads per block
COL_SHAPES = tuple((o, a, i) for i in (2, 255, 256, 257) for o in (1, 3) for a in (1, 2, 100))
MIDDLE_AXIS_SHAPE = (5, 67, 9)               # a 3-D tile scanned along its middle axis

# positions of a planted value inside a line of EDGE_A elements: inside a 64-chunk and on lanes 0 / 63 of a boundary
EDGE_A = 200
EDGE_POS = (0, 5, 62, 63, 64, 65, 127, 128, 199)


def _rng(*key):
  return np.random.RandomState([20150721] + [int(k) & 0x7fffffff for k in key])


def _freeze(x):
  x.setflags(write=False)
  return x


@functools.lru_cache(maxsize=None)
def data(shape, dtype, product, kind='mixed'):
  """A read-only [outer, A, inner] array.
  floats, sum:      mixed signs, magnitudes over 2^-20 .. 2^20, every second element nearly cancelling the one before.
  floats, product:  mixed signs, magnitudes 2^-2 .. 2^2 steered so that every prefix stays within 2^+-40.
  floats, 'whole':  whole values |x| <= 50 (sum: every partial sum stays far below 2^24) or +-1, +-2, +-0.5 (product:
                    powers of two): exactly representable in any order, so the result must be exact.
  integers, sum:    values over the whole width: every line wraps.
  integers, product: values in -3 .. 3 without 0 in line 0 (it wraps past the width), with zeros in the others."""
  dt = np.dtype(dtype)
  o, a, i = shape
  rng = _rng(o, a, i, dt.itemsize, dt.kind == 'f', product, len(kind))
  if dt.kind == 'f':
    if product:
      # exponents drawn in [-2, 2] (whole: -1, 0, 1), turned back whenever the running exponent leaves +-20
      e = rng.randint(-1, 2, size=shape).astype(np.float64) if kind == 'whole' else rng.uniform(-2, 2, size=shape)
      level = np.zeros((o, i))
      for k in range(a):
        e[:, k] = np.where(np.abs(level) > 20, -np.sign(level) * np.abs(e[:, k]), e[:, k])
        level += e[:, k]
      x = np.where(rng.rand(*shape) < 0.5, -1.0, 1.0) * 2.0 ** e
    elif kind == 'whole':
      x = rng.randint(-50, 51, size=shape).astype(np.float64)
    else:
      x = np.where(rng.rand(*shape) < 0.5, -1.0, 1.0) * 2.0 ** rng.uniform(-20, 20, size=shape) * rng.uniform(1, 2, size=shape)
      x[:, 1::2] = -x[:, 0:2 * (a // 2):2] * (1 + rng.uniform(-1e-3, 1e-3, size=x[:, 1::2].shape))
    return _freeze(x.astype(dt))
  info = np.iinfo(dt)
  if product:
    x = rng.randint(-3, 4, size=shape).astype(dt)
    first = x[0]
    first[first == 0] = 3
  else:
    x = rng.randint(info.min // 2, info.max // 2, size=shape, dtype=np.int64).astype(dt)
  return _freeze(x)


def numpy_scan(x, axis, product):
  """np.cumsum / np.cumprod in the input's own dtype (integers wrap; floats in NumPy's sequential order)."""
  with np.errstate(all='ignore'):
    return (np.cumprod if product else np.cumsum)(x, axis=axis, dtype=x.dtype)


def wide_scan(x, axis, product):
  """The scan accumulated in the next wider float type (float64 for float32, longdouble for float64)."""
  w = np.asarray(x, WIDER[np.dtype(x.dtype)])
  return (np.cumprod if product else np.cumsum)(w, axis=axis)


def float_bound(x, axis, product):
  """Per element: the absolute bound of a sum, the relative bound of a product."""
  dt = np.dtype(x.dtype)
  shape = [1] * x.ndim
  shape[axis] = x.shape[axis]
  j = np.arange(x.shape[axis], dtype=np.float64).reshape(shape)
  if product:
    return np.broadcast_to(j * EPS[dt], x.shape)
  return j * EPS[dt] * np.asarray(np.cumsum(np.abs(np.asarray(x, WIDER[dt])), axis=axis), np.float64)


def check_float(got, x, axis, product, label=''):
  """`got` within the derived bound of the wide reference, element by element; prints the worst ratio first."""
  got = np.asarray(got)
  assert got.dtype == x.dtype and got.shape == x.shape, (label, got.dtype, got.shape)
  ref = wide_scan(x, axis, product)
  bound = float_bound(x, axis, product)
  wide = WIDER[np.dtype(x.dtype)]
  if product:
    assert np.all(ref != 0) and np.all(np.isfinite(np.asarray(ref, np.float64))), 'a product line left the range'
    err = np.asarray(np.abs(np.asarray(got, wide) / ref - 1), np.float64)
  else:
    err = np.asarray(np.abs(np.asarray(got, wide) - ref), np.float64)
  with np.errstate(all='ignore'):
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
  print('%s: worst error / bound %.3g' % (label, float(ratio.max()) if ratio.size else 0.0))
  assert np.all(err <= bound), (label, float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))
  return float(ratio.max()) if ratio.size else 0.0


def check_exact(got, want, label=''):
  got = np.asarray(got)
  assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
  assert got.tobytes() == np.ascontiguousarray(want).tobytes(), (label, np.argwhere(got != want)[:5])


# ---------------------------------------------------------------------------------------------------- edges
@functools.lru_cache(maxsize=None)
def edge_lines(dtype, product, inner=1):
  """(clean [L, EDGE_A, inner], planted [L, EDGE_A, inner], plans): line l of `planted` is line l of `clean` with the
  edge plans[l] = (what, position[, second position]) planted in it.  Clean values are finite, 0.75 <= |x| <= 1.3.
    nan       a NaN at the position
    zero      (product) a zero at the position
    inf-inf   (sum) +inf at the first position, -inf at the second
    inf*zero  (product) +inf at the first position, 0 at the second"""
  dt = np.dtype(dtype)
  plans = []
  for p in EDGE_POS:
    plans.append(('nan', p))
    if product:
      plans.append(('zero', p))
  for p, q in ((0, 63), (5, 64), (62, 63), (63, 64), (64, 65), (63, 128), (127, 199)):
    plans.append(('inf*zero' if product else 'inf-inf', p, q))
  rng = _rng(dt.itemsize, product, inner, 77)
  size = (len(plans), EDGE_A, inner)
  clean = (np.where(rng.rand(*size) < 0.5, -1.0, 1.0) * rng.uniform(0.75, 1.3, size=size)).astype(dt)
  planted = np.array(clean)
  for l, plan in enumerate(plans):
    if plan[0] == 'nan':
      planted[l, plan[1]] = np.nan
    elif plan[0] == 'zero':
      planted[l, plan[1]] = 0
    else:
      planted[l, plan[1]] = np.inf
      planted[l, plan[2]] = 0 if product else -np.inf
  return _freeze(clean), _freeze(planted), tuple(plans)


def check_edges(got_clean, got_planted, plans, label=''):
  """The stated behaviour of every planted line, given the kernel's own result on the clean lines: positions in front
  of the edge keep their bits; behind a NaN everything is NaN; behind a zero every product is 0; from +inf on
  everything is infinite (a sum: +inf) until the -inf / the zero, and NaN from there on."""
  gc, gp = np.asarray(got_clean), np.asarray(got_planted)
  assert np.all(np.isfinite(gc)), label
  for l, plan in enumerate(plans):
    p = plan[1]
    assert gp[l, :p].tobytes() == gc[l, :p].tobytes(), (label, plan, 'positions in front of the edge changed')
    if plan[0] == 'nan':
      assert np.all(np.isnan(gp[l, p:])), (label, plan)
    elif plan[0] == 'zero':
      assert np.all(gp[l, p:] == 0), (label, plan)
    else:
      q = plan[2]
      assert np.all(np.isnan(gp[l, q:])), (label, plan)
      if plan[0] == 'inf-inf':
        assert np.all(gp[l, p:q] == np.inf), (label, plan)
      else:
        assert np.all(np.isinf(gp[l, p:q])), (label, plan)


@functools.lru_cache(maxsize=None)
def overflow_lines(dtype, inner=1):
  """[3, EDGE_A, inner] lines of one power of two each (b, -b, and b with every third element negative) whose cumprod
  overflows to +-inf: float32 b = 4 reaches 2^128 at position 63, float64 b = 2^6 reaches 2^1026 at position 170.
  Every partial product of a contiguous run is a power of two no larger than the prefix it belongs to, so any order
  gives np.cumprod's bits."""
  dt = np.dtype(dtype)
  big = 4.0 if dt == np.float32 else 2.0 ** 6
  x = np.full((3, EDGE_A, inner), big, dt)
  x[1] = -big
  x[2, ::3] = -big
  return _freeze(x)


# ---------------------------------------------------------------------------------------------------- operator
OP_WORKERS = (1, 3, 4)
# (shape, tile_hint): ragged tilings (the last tile along an axis is short) and one even tiling
OP_TILINGS = (((50, 37), (12, 5)), ((48, 20), (12, 5)), ((7, 130), (7, 64)))
OP_3D = ((6, 11, 5), (4, 4, 5))
REFUSED = (np.uint8, np.int8, np.int16, np.uint16, np.uint32, np.float16)


@functools.lru_cache(maxsize=None)
def op_input(shape, dtype, product):
  """Operator input: floats as data(); int32 / int64 small enough that nothing wraps in int64, the type NumPy scans
  both in (sums of |x| <= 1000; products of 38 factors |x| <= 3 among ones); bool about half set (product: 97 %)."""
  dt = np.dtype(dtype)
  rng = _rng(len(shape), shape[0], shape[-1], dt.itemsize, dt.kind == 'b', product)
  if dt.kind == 'f':
    flat = data((1, int(np.prod(shape)), 1), dt, product).reshape(shape)
    return _freeze(np.array(flat))
  if dt.kind == 'b':
    return _freeze(rng.rand(*shape) < (0.97 if product else 0.5))
  if product:
    x = np.ones(int(np.prod(shape)), dt)          # 38 factors other than 1: no prefix reaches 3^38 < 2^61
    x[rng.choice(x.size, 38, replace=False)] = rng.choice([-1, 2, -2, 3, -3], size=38)
    x = x.reshape(shape)
  else:
    x = rng.randint(-1000, 1001, size=shape).astype(dt)
  return _freeze(x)


def op_reference(x, axis, product):
  """What np.cumsum / np.cumprod returns (axis None: over the flattened array, in the array's shape)."""
  fn = np.cumprod if product else np.cumsum
  with np.errstate(all='ignore'):
    return fn(x, axis=axis).reshape(x.shape)


def op_check(got, x, axis, product, label=''):
  """The operator's result against NumPy: dtype always; integers and bool exactly; floats under the bound of a line
  that runs across the tiles (axis None: the one line of the flattened array)."""
  want = op_reference(x, axis, product)
  got = np.asarray(got)
  assert got.dtype == want.dtype, (label, got.dtype, want.dtype)
  assert got.shape == want.shape, (label, got.shape, want.shape)
  if np.dtype(x.dtype).kind != 'f':
    assert np.array_equal(got, want), (label, np.argwhere(got != want)[:5])
    return 0.0
  if axis is None:
    return check_float(got.reshape(-1), np.ascontiguousarray(x).reshape(-1), 0, product, label)
  return check_float(got, x, axis, product, label)


OP_DTYPES = (np.float32, np.int64, np.int32, np.bool_)


def run_operator_cases(sp, workers, dtype):
  """Every operator case of one dtype through `sp.scan` on the backend `sp` was initialised with."""
  for shape, hint in OP_TILINGS[:1] + (OP_3D,) + (OP_TILINGS[1:] if np.dtype(dtype) == np.float32 else ()):
    for product in (False, True):
      x = op_input(shape, dtype, product)
      X = sp.from_numpy(np.array(x), tile_hint=list(hint))
      pair = (np.prod, np.cumprod) if product else (np.sum, np.cumsum)
      for axis in (None, 0, 1) + ((2,) if len(shape) == 3 else ()):
        if axis is None and len(shape) == 3:
          continue        # (the flattened scan is the reference's 2-D formulation, scan.py:52-57)
        got = sp.scan(X, pair[0], pair[1], axis=axis).glom()
        op_check(got, x, axis, product, '%d workers %s %s axis %s %s' % (workers, shape, np.dtype(dtype).name, axis,
                                                                          'prod' if product else 'sum'))


def run_refusals(sp, backend):
  """uint8 (np.cumsum would make uint64, which is no tile dtype) and the five narrow types: a TypeError, nothing run."""
  import pytest
  for dtype in REFUSED:
    before = backend.launches
    with pytest.raises(TypeError):
      x = sp.from_numpy(np.arange(40).reshape(8, 5).astype(dtype), tile_hint=[4, 5])
      before = backend.launches
      sp.scan(x, axis=0).glom()
    assert backend.launches == before, dtype
    with pytest.raises(TypeError):
      x = sp.from_numpy(np.arange(40).reshape(8, 5).astype(dtype), tile_hint=[4, 5])
      before = backend.launches
      sp.scan(x, np.prod, np.cumprod, axis=None).glom()
    assert backend.launches == before, dtype
