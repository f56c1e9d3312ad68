"""Cases of integer-array indexing `x[idx]` (expr/filter.py) and of its tile kernel sp_gather_rows (csrc/update.hip).
Pure NumPy; the reference is NumPy's own `src[idx]`, exact.

The kernel moves a row as words of 16, 4, 2 or 1 bytes: the widest that the row length, the row stride and both base
pointers are multiples of.  KERNEL_ROWS names, per row length in bytes, an element type and a row shape that give it.
"""
import functools

import numpy as np

# row bytes -> (dtype, shape of one row): 1 3 | 2 6 | 4 12 2068 | 16 48 are the byte, 2-byte, 4-byte and 16-byte paths
KERNEL_ROWS = (
    (1, np.uint8, ()), (3, np.int8, (3,)), (2, np.uint8, (2,)), (6, np.int16, (3,)), (4, np.float32, ()),
    (12, np.int32, (3,)), (16, np.float64, (2,)), (48, np.float32, (3, 4)), (2068, np.float32, (517,)),
)
N_SRC = 37
# negative, repeated, unsorted; the last and (by its negative index) the second row; no -N_SRC (see gather tests)
INDEX = np.array([5, -1, 0, 36, 5, 5, -36, 17, 2, -9, 30, 1, 36, 0, -1], np.int64)
INDEX.setflags(write=False)
# more than 8192 blocks of 256 words: the grid strides
BIG = (4100, 300, 517)


@functools.lru_cache(maxsize=None)
def source(n, dtype, row_shape, seed=0):
  """A read-only [n, *row_shape] array of random bytes (bool: random bits; floats: normal deviates), so that a row
  taken from the wrong place, or a byte from the wrong offset, shows."""
  dt = np.dtype(dtype)
  rng = np.random.RandomState([20150722, n, dt.itemsize, len(row_shape), seed])
  shape = (n,) + tuple(row_shape)
  if dt.kind == 'b':
    x = rng.rand(*shape) < 0.5
  elif dt.kind == 'f':
    x = rng.standard_normal(shape).astype(dt)
  else:
    x = rng.randint(0, 256, size=shape + (dt.itemsize,)).astype(np.uint8).view(dt).reshape(shape)
  x.setflags(write=False)
  return x


def row_bytes(x):
  return int(np.prod(x.shape[1:], dtype=np.int64)) * x.dtype.itemsize


@functools.lru_cache(maxsize=None)
def big_index():
  n_idx, n_src, _ = BIG
  idx = np.random.RandomState(20150723).randint(-n_src + 1, n_src, size=n_idx).astype(np.int64)
  idx.setflags(write=False)
  return idx


# ---- the operator: (source shape, dtype) of x, every one at 1, 3 and 4 workers
OP_WORKERS = (1, 3, 4)
OP_SOURCES = (((10, 4), np.float32), ((10,), np.float64), ((10, 3), np.bool_), ((33,), np.uint8), ((21, 5), np.uint8),
              ((20, 3, 5), np.int64), ((10,), np.bool_))
OUT_OF_RANGE = ((-11, 2), (10,), (0, 10), (-11,), (3, 1, 2**40), (-2**40,))       # for 10 rows


def run_operator_cases(sp, extra_dtypes=()):
  """x[idx] == NumPy's for every source, with negative, repeated and unsorted indices that include -n and n - 1,
  a single index, and an index that lives in a distributed array."""
  sources = OP_SOURCES + tuple(((19, 3), dt) for dt in extra_dtypes)
  for shape, dtype in sources:
    x = source(shape[0], dtype, shape[1:], seed=1)
    n = shape[0]
    rng = np.random.RandomState(n)
    idx = np.concatenate([[-n, n - 1, -1, 0, 3, 3], rng.randint(-n, n, size=21)]).astype(np.int64)
    X = sp.from_numpy(np.array(x))
    for ix in (idx, idx[:1], np.array([n - 1]), idx.astype(np.int32)):
      got = X[ix].glom()
      assert got.dtype == x.dtype and got.shape == x[ix].shape, (shape, dtype, got.dtype, got.shape)
      assert np.array_equal(got, x[ix]), (shape, dtype)
    pos = idx % n
    assert np.array_equal(X[sp.from_numpy(pos)].glom(), x[pos]), (shape, dtype)


def run_range_checks(sp, backend):
  """NumPy's IndexError for anything outside [-n, n), before the source is fetched or anything is launched for it;
  the edges of the range pass."""
  import pytest
  for shape, dtype in (((10, 4), np.float32), ((10,), np.int64), ((10, 3), np.bool_)):
    x = source(10, dtype, shape[1:], seed=2)
    X = sp.from_numpy(np.array(x))
    X.evaluate()
    for bad in OUT_OF_RANGE:
      with pytest.raises(IndexError):
        x[np.array(bad)]                                   # NumPy's own verdict
      for ix in (np.array(bad, np.int64), sp.from_numpy(np.array(bad, np.int64))):
        e = X[ix]
        own = 0
        if not isinstance(ix, np.ndarray):
          # a distributed index has to come to the host to be checked: that fetch, and nothing else, may run
          before = backend.launches
          ix.glom()
          own = backend.launches - before
        before = backend.launches
        with pytest.raises(IndexError, match='out of bounds'):
          e.glom()
        assert backend.launches - before in (0, own), (bad, type(ix).__name__, 'something ran before the refusal')
    edge = np.array([-10, 9])
    assert np.array_equal(X[edge].glom(), x[edge])
