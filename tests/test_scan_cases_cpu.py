"""What the scan tests stand on, without a GPU: the references, bounds and cases of tests/scan_cases.py hold for NumPy
itself and for a NumPy restatement of the row kernel's order (64-lane shuffle scan, carry from lane 63), and they
reject that restatement with a wrong carry.  The operator (expr/scan.py) runs here on the NumPy oracle backend under
the checks the GPU run uses (tests/test_scan_gpu.py)."""
import numpy as np
import pytest

import spartan_amd as sp
from tests import scan_cases as sc

ids = lambda d: np.dtype(d).name        # noqa: E731
OPS = (False, True)
op_ids = lambda p: 'prod' if p else 'sum'        # noqa: E731


def shuffle_scan_rows(x, product, carry_lane=63):
  """The row kernel's order in the input's own dtype: per line, chunks of 64; inside a chunk a Hillis-Steele scan
  (lane l combines with lane l - off, off = 1, 2, .. 32; lanes past the end hold the identity); the chunk's result is
  combined with the carry, and the next carry is lane `carry_lane` of it."""
  dt = x.dtype
  op = np.multiply if product else np.add
  ident = dt.type(1 if product else 0)
  o, a = x.shape
  out = np.empty_like(x)
  with np.errstate(all='ignore'):
    for a0 in range(0, a, 64):
      v = np.full((o, 64), ident, dt)
      n = min(64, a - a0)
      v[:, :n] = x[:, a0:a0 + n]
      off = 1
      while off < 64:
        v[:, off:] = op(v[:, :-off], v[:, off:])
        off <<= 1
      v = op(carry[:, None], v) if a0 else v
      out[:, a0:a0 + n] = v[:, :n]
      carry = v[:, carry_lane].copy()
  return out


@pytest.mark.parametrize('product', OPS, ids=op_ids)
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
def test_float_bound_holds_for_two_orders_and_rejects_a_wrong_carry(dtype, product):
  caught = tried = 0
  for shape in sc.ROW_SHAPES + (sc.ROW_STRIDE_SHAPE,):
    x = sc.data(shape, dtype, product)
    lines = x.reshape(shape[0], shape[1])
    label = '%s %s' % (shape, np.dtype(dtype).name)
    sc.check_float(sc.numpy_scan(x, 1, product), x, 1, product, 'numpy ' + label)           # sequential order
    sc.check_float(shuffle_scan_rows(lines, product).reshape(shape), x, 1, product, 'shuffle ' + label)
    if shape[1] > 64 and shape[0] < 10:
      # an element lost at a chunk boundary shows unless it is small beside its neighbours (the exponent range is
      # wide on purpose); the whole-valued lines of the next test catch it at every shape
      tried += 1
      try:
        sc.check_float(shuffle_scan_rows(lines, product, carry_lane=62).reshape(shape), x, 1, product, 'lane 62 ' + label)
      except AssertionError:
        caught += 1
  assert tried == 20 and caught >= 15, (tried, caught)
  # the data is what the module says it is: mixed signs, cancellation, a wide exponent range
  x = sc.data((3, 1000, 1), dtype, product)
  assert (x > 0).any() and (x < 0).any()
  if not product:
    mag = np.abs(x.astype(np.float64))
    assert mag.max() / mag.min() > 2.0 ** 30
    assert np.abs(np.asarray(sc.wide_scan(x, 1, False), np.float64)).min() < 1e-3 * mag.sum(axis=1).min()


@pytest.mark.parametrize('product', OPS, ids=op_ids)
@pytest.mark.parametrize('dtype', sc.DTYPES, ids=ids)
def test_whole_values_and_integers_are_exact_in_any_order(dtype, product):
  wrapped = False
  for shape in sc.ROW_SHAPES:
    floating = np.dtype(dtype).kind == 'f'
    x = sc.data(shape, dtype, product, 'whole') if floating else sc.data(shape, dtype, product)
    want = sc.numpy_scan(x, 1, product)
    lines = x.reshape(shape[0], shape[1])
    sc.check_exact(shuffle_scan_rows(lines, product).reshape(shape), want, str(shape))
    if shape[1] > 64 and not product and np.all(lines[:, 63] != 0):
      # (a lost element shows in a sum unless it is 0; in a product a lost 1 or a zero in front of it hides it)
      assert shuffle_scan_rows(lines, product, carry_lane=62).tobytes() != want.tobytes()
    if floating:
      big = np.abs(np.asarray(sc.wide_scan(x, 1, product), np.float64)).max()
      assert big < sc.EXACT_BELOW[np.dtype(dtype)]
    else:
      # the true value, in Python integers, leaves the width: the expected line really wraps
      line = [int(v) for v in lines[0]]
      acc, true = (1 if product else 0), []
      for v in line:
        acc = acc * v if product else acc + v
        true.append(acc)
      info = np.iinfo(dtype)
      if any(t < info.min or t > info.max for t in true):
        wrapped = True
        bits = 8 * np.dtype(dtype).itemsize
        assert [int(v) for v in want.reshape(shape[0], shape[1])[0]] == \
            [((t + (1 << (bits - 1))) % (1 << bits)) - (1 << (bits - 1)) for t in true]
  assert wrapped or np.dtype(dtype).kind == 'f'


@pytest.mark.parametrize('dtype', sc.DTYPES, ids=ids)
def test_column_shapes_reference(dtype):
  # np.cumsum along a middle axis is sequential per line: the same bits as a Python loop over the axis
  for shape in (sc.MIDDLE_AXIS_SHAPE, (3, 100, 257)):
    for product in OPS:
      x = sc.data(shape, dtype, product)
      want = sc.numpy_scan(x, 1, product)
      acc = x[:, 0].copy()
      with np.errstate(all='ignore'):
        for k in range(shape[1]):
          if k:
            acc = (acc * x[:, k] if product else acc + x[:, k]).astype(dtype)
          assert acc.tobytes() == np.ascontiguousarray(want[:, k]).tobytes(), (shape, k)


@pytest.mark.parametrize('inner', (1, 3))
@pytest.mark.parametrize('product', OPS, ids=op_ids)
@pytest.mark.parametrize('dtype', sc.FLOATS, ids=ids)
def test_edge_lines(dtype, product, inner):
  clean, planted, plans = sc.edge_lines(dtype, product, inner)
  assert clean.shape == planted.shape == (len(plans), sc.EDGE_A, inner)
  kinds = set(p[0] for p in plans)
  assert kinds == ({'nan', 'zero', 'inf*zero'} if product else {'nan', 'inf-inf'})
  assert set(p[1] for p in plans if p[0] == 'nan') == set(sc.EDGE_POS) and {0, 63, 64} <= set(sc.EDGE_POS)
  sc.check_edges(sc.numpy_scan(clean, 1, product), sc.numpy_scan(planted, 1, product), plans, 'numpy')
  if inner == 1:
    rows = lambda v: shuffle_scan_rows(v.reshape(len(plans), sc.EDGE_A), product).reshape(v.shape)    # noqa: E731
    sc.check_edges(rows(clean), rows(planted), plans, 'shuffle')
    with pytest.raises(AssertionError):
      bad = lambda v: shuffle_scan_rows(v.reshape(len(plans), sc.EDGE_A), product, 62).reshape(v.shape)    # noqa: E731
      sc.check_edges(rows(clean), bad(planted), plans, 'lane 62')
  if product:
    x = sc.overflow_lines(dtype, inner)
    want = sc.numpy_scan(x, 1, True)
    assert np.isinf(want[:, -1]).all() and np.isfinite(want[:, 0]).all()
    assert (want[1, -2:, 0] == [-np.inf, np.inf]).all() or (want[1, -2:, 0] == [np.inf, -np.inf]).all()
    first_inf = int(np.argmax(np.isinf(want[0, :, 0])))
    assert first_inf == (63 if np.dtype(dtype) == np.float32 else 170)
    if inner == 1:
      sc.check_exact(shuffle_scan_rows(x.reshape(3, sc.EDGE_A), True).reshape(x.shape), want, 'overflow')


# ------------------------------------------------------------------------------------------------ the operator
@pytest.mark.parametrize('dtype', sc.OP_DTYPES, ids=ids)
@pytest.mark.parametrize('workers', sc.OP_WORKERS)
def test_operator_on_the_numpy_backend(workers, dtype):
  from oracle.np_backend import NumpyBackend
  sp.initialize(backend=NumpyBackend(), num_workers=workers)
  try:
    sc.run_operator_cases(sp, workers, dtype)
  finally:
    sp.shutdown()


def test_operator_refusals_on_the_numpy_backend():
  from oracle.np_backend import NumpyBackend
  ctx = sp.initialize(backend=NumpyBackend(), num_workers=3)
  try:
    sc.run_refusals(sp, ctx.backend)
  finally:
    sp.shutdown()


def test_operator_cases_are_what_they_claim():
  ragged = [any(s % h for s, h in zip(shape, hint)) for shape, hint in sc.OP_TILINGS + (sc.OP_3D,)]
  assert ragged == [True, False, True, True]          # short last tiles; one even tiling beside them
  b = sc.op_input((50, 37), np.bool_, False)
  assert b.dtype == np.bool_ and 0.3 < b.mean() < 0.7
  assert sc.op_reference(b, 1, False).dtype == np.int64 and sc.op_reference(b, None, True).dtype == np.int64
  i = sc.op_input((50, 37), np.int32, False)
  assert sc.op_reference(i, 0, False).dtype == np.int64 and sc.op_reference(i, 0, True).dtype == np.int64
  assert np.abs(np.cumsum(i.astype(np.int64))).max() < 2 ** 31
  big = np.abs(np.cumprod(sc.op_input((50, 37), np.int32, True).astype(object))).max()
  assert 2 ** 31 < big < 2 ** 63                  # past int32 (the result is int64), inside int64
