"""Inputs, term-by-term models and structural references for the sparse tile kernels (csrc/sparse.hip,
csrc/spmv_blocked.hip).  Pure NumPy plus scipy, no GPU import.

The kernels promise ORDERS of summation (include/spartan_hip.h), and whole-valued test data cannot see an order.  The
values here are sign * 2^U(-8, 8) * U(1, 2): adding them in another order changes bits.  Every model rounds each
product and each addition to the tile's dtype (NumPy arithmetic on float32 / float64 arrays does; the library is built
with -ffp-contract=off, so a product is rounded before it is added), and the GPU tests compare bit patterns.

  coo_sum_list_order    sp_coo_to_csr: a cell's entries are added one after the other in list order
  spmv_rows_sequential  n == 1, planned kernel with a longest row <= 65, and the blocked kernel: s = 0, s += a * x in
                        storage order, y = s or y0 + s (the row's sum meets y0 LAST: the existing blocked-kernel test
                        pins y0 + (A x) too)
  spmv_chunked          n == 1, stream kernel + fix-up and the planned kernel's long-row mode: chunks of 2048 stored
                        entries; a row's part inside the chunk it starts in is summed sequentially (y = y0 + s), each
                        later chunk's head of the row as 64 lane-strided partial sums and a butterfly, and the carries
                        are added to y in chunk order
  spmv_lanes            n == 1, lanes-per-row kernel: lane g of G adds entries a + g, a + g + G, ..., a butterfly over G
                        lanes, y = y0 + acc
  spmm_rows_sequential  n > 1: acc = C0 or 0, acc += a * B[k, :] in storage order (C0 comes FIRST here)
  spgemm_k_ascending    expansion in A's storage order, then coo_sum_list_order

Bound used by the CPU self-checks (derived, not measured; tests/scan_cases.py): a sum of `len` rounded products in any
order is within len * eps * sum|a||x| of the sum accumulated in the next wider type.
"""
import functools

import numpy as np
import scipy.sparse as sps

LD = np.longdouble
FLOATS = (np.float32, np.float64)
EPS = {np.dtype(np.float32): 2.0 ** -23, np.dtype(np.float64): 2.0 ** -52}
WIDER = {np.dtype(np.float32): np.float64, np.dtype(np.float64): LD}
BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}

SPMV_CH = 2048          # stored entries per chunk of the stream / planned kernels
SPMV_SPILL = 64         # entries behind a chunk the planned kernel loads: whole rows up to SPMV_SPILL + 1
SCAN_CHUNK = 4096       # elements per block of the exclusive scan behind sp_coo_to_csr / sp_spgemm_count
GRID_CAP = 256 * 8 * 4  # grid_for(): SP_CUS * SP_BLOCKS_PER_CU * 4 workgroups at most


def _rng(*key):
  return np.random.RandomState([20151103] + [int(k) & 0x7fffffff for k in key])


def _freeze(*arrays):
  for a in arrays:
    a.setflags(write=False)
  return arrays[0] if len(arrays) == 1 else arrays


def bits(a):
  """The bit patterns of a float array (what the GPU tests compare)."""
  a = np.ascontiguousarray(a)
  return a.view(BITS[np.dtype(a.dtype)])


def assert_same_bits(got, want, label=''):
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
  np.testing.assert_array_equal(bits(got), bits(want), err_msg=str(label))


def assert_same_bits_nan_aware(got, want, label=''):
  """NaNs at the same positions (the payload of a NaN is not part of any contract), the same bits everywhere else."""
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg='%s: NaN positions' % (label,))
  ok = ~np.isnan(want)
  np.testing.assert_array_equal(bits(got)[ok], bits(want)[ok], err_msg=str(label))


# ---------------------------------------------------------------------------------------------------- values
def real_values(n, dtype, *key):
  """n values sign * 2^U(-8, 8) * U(1, 2): mixed signs and magnitudes, so that the order of a sum shows in its bits."""
  rng = _rng(77, n, np.dtype(dtype).itemsize, *key)
  v = np.where(rng.rand(n) < 0.5, -1.0, 1.0) * 2.0 ** rng.uniform(-8, 8, size=n) * rng.uniform(1, 2, size=n)
  return v.astype(dtype)


def whole_values(n, dtype, *key):
  """n whole values in -4 .. 4: every sum of them is exact in any order."""
  return _rng(78, n, *key).randint(-4, 5, size=n).astype(dtype)


# ---------------------------------------------------------------------------------------------------- building blocks
def _segment_sums(p, starts, lens):
  """s[i] = ((0 + p[starts[i]]) + p[starts[i] + 1]) + ... over lens[i] terms, every addition rounded to p.dtype."""
  starts, lens = np.asarray(starts, np.int64), np.asarray(lens, np.int64)
  out = np.zeros(lens.shape, p.dtype)
  with np.errstate(all='ignore'):
    for i in np.nonzero(lens > 128)[0]:         # few long segments: np.cumsum adds one after the other
      out[i] = np.cumsum(p[starts[i]:starts[i] + lens[i]], dtype=p.dtype)[-1]
    active = np.nonzero((lens > 0) & (lens <= 128))[0]
    t = 0
    while active.size:
      out[active] = out[active] + p[starts[active] + t]
      t += 1
      active = active[lens[active] > t]
  return out


def _butterfly(s):
  """s[..., l] += s[..., l ^ off] for off = W / 2 .. 1 over the last axis (the __shfl_xor tree); lane 0's result."""
  w = s.shape[-1]
  lane = np.arange(w)
  off = w // 2
  with np.errstate(all='ignore'):
    while off > 0:
      s = s + s[..., lane ^ off]
      off >>= 1
  return s[..., 0]


def _lane_strided_sum(p, w=64):
  """One wavefront over p: lane l adds p[l], p[l + w], ... to 0, then the butterfly."""
  n = p.size
  pad = np.zeros((-n) % w, p.dtype)          # (a lane that runs out of terms adds nothing: s + 0 == s)
  q = np.concatenate([p, pad]).reshape(-1, w)
  s = np.zeros(w, p.dtype)
  with np.errstate(all='ignore'):
    for row in q:
      s = s + row
  return _butterfly(s)


def _products(csr, x):
  """The rounded products a * x[col] of every stored entry (x None: the values themselves -- row sums)."""
  if x is None:
    return np.array(csr.data)
  x = np.asarray(x).reshape(-1)
  assert x.dtype == csr.data.dtype and x.size == csr.shape[1]
  with np.errstate(all='ignore'):
    return csr.data * x[csr.indices]


def _with_y0(s, y0):
  if y0 is None:
    return s
  with np.errstate(all='ignore'):
    return np.asarray(y0).reshape(-1) + s


# ---------------------------------------------------------------------------------------------------- models
def coo_sum_list_order(rows, cols, vals, shape, reverse=False):
  """Canonical CSR (indptr int64, indices int32, data) of a COO list: entries with row < 0 dropped, every cell summed
  one entry after the other in list order (`reverse`: in reversed list order -- the wrong order the CPU tests try)."""
  rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals)
  nrows, ncols = int(shape[0]), int(shape[1])
  keep = np.nonzero(rows >= 0)[0]
  if reverse:
    keep = keep[::-1]
  key = rows[keep] * ncols + cols[keep]
  order = np.argsort(key, kind='stable')
  key, v = key[order], vals[keep][order]
  head = np.ones(key.size, bool)
  head[1:] = key[1:] != key[:-1]
  starts = np.nonzero(head)[0]
  lens = np.diff(np.append(starts, key.size))
  data = _segment_sums(v, starts, lens)
  cells = key[starts]
  indptr = np.searchsorted(cells, np.arange(nrows + 1, dtype=np.int64) * ncols).astype(np.int64)
  return indptr, (cells % max(ncols, 1)).astype(np.int32), data.astype(vals.dtype)


def coo_cell_terms(rows, cols, shape):
  """Number of list entries of every cell of coo_sum_list_order's result, in its order."""
  rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
  key = np.sort((rows * int(shape[1]) + cols)[rows >= 0])
  return np.unique(key, return_counts=True)[1]


def spmv_rows_sequential(csr, x, y0=None):
  lens = np.diff(csr.indptr)
  return _with_y0(_segment_sums(_products(csr, x), csr.indptr[:-1], lens), y0)


def spmv_chunked(csr, x, y0=None):
  p = _products(csr, x)
  ptr = np.asarray(csr.indptr, np.int64)
  a, b = ptr[:-1], ptr[1:]
  nnz = int(ptr[-1])
  first_end = np.minimum(b, np.minimum((a // SPMV_CH + 1) * SPMV_CH, nnz))
  y = _with_y0(_segment_sums(p, a, first_end - a), y0)
  y = np.array(y)
  with np.errstate(all='ignore'):
    for r in np.nonzero(b > first_end)[0]:
      for e0 in range(int(first_end[r]), int(b[r]), SPMV_CH):       # first_end of a spanning row is a chunk boundary
        y[r] = y[r] + _lane_strided_sum(p[e0:min(e0 + SPMV_CH, int(b[r]))])
  return y


def rows_spanning_chunks(csr):
  ptr = np.asarray(csr.indptr, np.int64)
  a, b = ptr[:-1], ptr[1:]
  return np.nonzero(b > (a // SPMV_CH + 1) * SPMV_CH)[0]


def spmv_lanes(csr, x, G, y0=None):
  p = _products(csr, x)
  ptr = np.asarray(csr.indptr, np.int64)
  lens = np.diff(ptr)
  rows = np.nonzero(lens > 0)[0]
  acc = np.zeros((rows.size, G), p.dtype)
  g = np.arange(G)
  a, n = ptr[rows], lens[rows]
  with np.errstate(all='ignore'):
    for t in range(int(-(-n.max() // G)) if rows.size else 0):
      at = t * G + g[None, :]                         # [rows, G] position inside the row
      live = at < n[:, None]
      term = np.where(live, p[np.where(live, a[:, None] + at, 0)], p.dtype.type(0))
      acc = acc + term
  s = np.zeros(lens.size, p.dtype)
  s[rows] = _butterfly(acc) if rows.size else 0
  return _with_y0(s, y0)


def spmm_rows_sequential(csr, B, C0=None):
  B = np.asarray(B)
  assert B.dtype == csr.data.dtype and B.shape[0] == csr.shape[1]
  ptr = np.asarray(csr.indptr, np.int64)
  lens = np.diff(ptr)
  acc = np.zeros((csr.shape[0], B.shape[1]), B.dtype) if C0 is None else np.array(C0, B.dtype)
  active = np.nonzero(lens > 0)[0]
  t = 0
  with np.errstate(all='ignore'):
    while active.size:
      e = ptr[active] + t
      acc[active] = acc[active] + csr.data[e][:, None] * B[csr.indices[e]]
      t += 1
      active = active[lens[active] > t]
  return acc


def spgemm_expand(a, b):
  """(rows, cols, products, offs) of the expansion step: A's entries in storage order, each against its row of B;
  offs[t] = number of products before A's entry t, offs[nnz_a] = their total."""
  counts = np.diff(b.indptr)[a.indices].astype(np.int64)
  offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
  total = int(offs[-1])
  rows_a = csr_rows_ref(a.indptr, a.nnz)
  within = np.arange(total, dtype=np.int64) - np.repeat(offs[:-1], counts)
  src = np.repeat(np.asarray(b.indptr, np.int64)[a.indices], counts) + within
  with np.errstate(all='ignore'):
    vals = np.repeat(a.data, counts) * b.data[src]
  return np.repeat(rows_a, counts).astype(np.int32), b.indices[src].astype(np.int32), vals, offs


def spgemm_k_ascending(a, b):
  rows, cols, vals, _ = spgemm_expand(a, b)
  return coo_sum_list_order(rows, cols, vals, (a.shape[0], b.shape[1]))


# ---------------------------------------------------------------------------------------------------- bound
def wide_spmv(csr, x, y0=None):
  """A x (+ y0) accumulated in the next wider type, and sum |a||x| (+ |y0|) as float64."""
  wide = WIDER[np.dtype(csr.data.dtype)]
  xw = np.ones(csr.shape[1], wide) if x is None else np.asarray(x, wide).reshape(-1)
  terms = np.asarray(csr.data, wide) * xw[csr.indices]
  ref = np.zeros(csr.shape[0], wide)
  mag = np.zeros(csr.shape[0], wide)
  np.add.at(ref, csr_rows_ref(csr.indptr, csr.nnz), terms)
  np.add.at(mag, csr_rows_ref(csr.indptr, csr.nnz), np.abs(terms))
  if y0 is not None:
    ref = ref + np.asarray(y0, wide).reshape(-1)
    mag = mag + np.abs(np.asarray(y0, wide).reshape(-1))
  return ref, np.asarray(mag, np.float64)


def check_spmv_bound(got, csr, x, y0=None, label=''):
  """|got - wide| <= len * eps * sum|a||x| row by row, len = the row's terms (+ 1 with y0)."""
  ref, mag = wide_spmv(csr, x, y0)
  terms = np.diff(csr.indptr) + (1 if y0 is not None else 0)
  err = np.asarray(np.abs(np.asarray(got, ref.dtype).reshape(-1) - ref), np.float64)
  bound = terms * EPS[np.dtype(csr.data.dtype)] * mag
  assert np.all(err <= bound), (label, int(np.argmax(err - bound)))


# ---------------------------------------------------------------------------------------------------- structure
def csr_rows_ref(indptr, nnz):
  rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int32), np.diff(indptr))
  assert rows.size == nnz
  return rows


def coo_box_ref(rows, cols, r0, r1, c0, c1, dr, dc, drop_inside):
  """sp_coo_box: dropped entries (row < 0) stay as they are; an entry the box drops gets row -1 and keeps its column."""
  rows, cols = np.array(rows, np.int32), np.array(cols, np.int32)
  live = rows >= 0
  inside = (rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1)
  drop = live & (inside == bool(drop_inside))
  keep = live & ~drop
  rows[drop] = -1
  rows[keep] += np.int32(dr)
  cols[keep] += np.int32(dc)
  return rows, cols


def coo_reshape_ref(rows, cols, old_cols, offset, new_rows, new_cols):
  """sp_coo_reshape in 64-bit integers: linear position row * old_cols + col - offset, re-split by new_cols."""
  r64, c64 = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
  rows, cols = np.array(rows, np.int32), np.array(cols, np.int32)
  live = r64 >= 0
  lin = r64 * int(old_cols) + c64 - int(offset)
  keep = live & (lin >= 0) & (lin < int(new_rows) * int(new_cols))
  rows[live & ~keep] = -1
  rows[keep] = (lin[keep] // int(new_cols)).astype(np.int32)
  cols[keep] = (lin[keep] % int(new_cols)).astype(np.int32)
  return rows, cols


def scatter_ref(csr, out, row0, col0, mode, mask=None):
  """sp_csr_scatter on host copies: (out, mask) after mode 0 assign / 1 add / 2 first write where the mask is clear."""
  out = np.array(out)
  mask = None if mask is None else np.array(mask)
  r = csr_rows_ref(csr.indptr, csr.nnz).astype(np.int64) + row0
  c = csr.indices.astype(np.int64) + col0
  with np.errstate(all='ignore'):
    if mode == 0:
      out[r, c] = csr.data
    elif mode == 1:
      out[r, c] = out[r, c] + csr.data
    else:
      seen = mask[r, c] != 0
      out[r, c] = np.where(seen, out[r, c] + csr.data, csr.data)
      mask[r, c] = 1
  return out, mask


# ---------------------------------------------------------------------------------------------------- builders
def csr_from_lens(lens, ncols, dtype, key=0, whole=False, avoid=()):
  """A CSR matrix (scipy, canonical) with the given row lengths, distinct ascending columns inside a row (none from
  `avoid`) and real_values (or whole_values)."""
  lens = np.asarray(lens, np.int64)
  rng = _rng(5, lens.size, int(lens.sum()), ncols, key)
  allowed = np.setdiff1d(np.arange(ncols, dtype=np.int64), np.asarray(avoid, np.int64))
  assert lens.max(initial=0) <= allowed.size
  indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
  indices = np.empty(int(indptr[-1]), np.int32)
  for r in np.nonzero(lens)[0]:
    n = int(lens[r])
    pick = rng.choice(allowed.size, size=n, replace=False) if n * 4 < allowed.size else rng.permutation(allowed.size)[:n]
    indices[indptr[r]:indptr[r + 1]] = np.sort(allowed[pick])
  nnz = indices.size
  data = whole_values(nnz, dtype, key) if whole else real_values(nnz, dtype, key)
  m = sps.csr_matrix((data, indices, indptr), shape=(lens.size, ncols))
  _freeze(m.data, m.indices, m.indptr)
  return m


def vector(n, dtype, key=0, whole=False):
  return _freeze((whole_values if whole else real_values)(n, dtype, 9, key))


def fill_lens(total, longest, key=0, exact=True, shortest=0):
  """Row lengths in shortest .. longest that add up to `total`, empty rows mixed in (shortest == 0); with `exact` one
  row (when total allows) is exactly `longest` long."""
  rng = _rng(6, total, longest, key)
  lens, left = [], total
  if exact and total >= longest:
    lens.append(longest)
    left -= longest
  while left > 0:
    n = int(min(left, rng.randint(shortest, longest + 1)))
    if shortest == 0 and rng.rand() < 0.15:
      n = 0
    lens.append(n)
    left -= n
  order = rng.permutation(len(lens))
  return [lens[i] for i in order]


@functools.lru_cache(maxsize=None)
def planned_whole_lens():
  """name -> row lengths, longest row <= 65: the planned kernel sums whole rows in the chunk they start in."""
  cases = {}
  # a row of exactly SPMV_SPILL + 1 = 65 entries that starts on a chunk's LAST entry: prod[2047 .. 2112), the end of the buffer
  cases['row65_starts_at_2047'] = [0] + fill_lens(2047, 60, 1, exact=False) + [65, 0, 3, 65, 1] + fill_lens(700, 65, 2)
  cases['row64_starts_at_2047'] = fill_lens(2047, 64, 3) + [64, 0, 0, 7] + fill_lens(300, 64, 4, exact=False)
  # rows ending exactly at 2048 / 4096, empty rows before, at and after the boundary
  cases['rows_end_at_boundary'] = ([0, 0] + fill_lens(2048 - 65, 65, 5, exact=False) + [0, 65, 0, 0] +
                                   fill_lens(2048 - 1, 50, 6, exact=False) + [1, 0, 0, 0, 9, 0])
  cases['longest_is_1'] = [0, 0] + [1, 1, 0, 1] * 700 + [0]
  for nnz in (1, 2047, 2048, 2049, 4096 + 64, 3 * 2048 + 5):
    cases['nnz_%d' % nnz] = [0] + fill_lens(nnz, min(65, nnz), nnz, exact=nnz >= 65) + [0, 0]
  for name, lens in cases.items():
    assert max(lens) <= SPMV_SPILL + 1, name
  assert max(cases['row65_starts_at_2047']) == 65 and max(cases['longest_is_1']) == 1
  at = int(np.cumsum([0] + cases['row65_starts_at_2047'])[cases['row65_starts_at_2047'].index(65)])
  assert at == SPMV_CH - 1
  at = int(np.cumsum([0] + cases['row64_starts_at_2047'])[len(fill_lens(2047, 64, 3))])
  assert at == SPMV_CH - 1
  return cases


@functools.lru_cache(maxsize=None)
def long_row_lens():
  """name -> row lengths with a longest row >= 66: partial sums per chunk and carries.  The names in ORDER_PINNING hold
  at least 20 rows that span chunks."""
  cases = {}
  for name, lens in planned_whole_lens().items():
    if name.startswith('row6') or name == 'rows_end_at_boundary':
      at = lens.index(max(lens))
      cases[name + '_and_66'] = lens[:at] + [66] + lens[at + 1:] if max(lens) == 65 else lens + [66]
  # 30 chunks of rows of 30 .. 66 entries: nearly every chunk boundary cuts a row
  cases['straddle_66'] = fill_lens(30 * SPMV_CH, 66, 7, shortest=30)
  # rows of 2049, 4096 and 5000 entries over 2 .. 4 chunks, one starting exactly on a boundary (entry 2048 after the
  # 2048-entry row), two carried rows in consecutive chunks, empty rows around them
  cases['rows_2049_4096_5000'] = ([2048, 2049, 0, 4096, 3, 5000, 0, 0, 2049, 2049, 40] * 3 +
                                  [2047, 2049, 4096, 0, 1, 5000] * 3 + [0])
  return cases


ORDER_PINNING_LONG = ('straddle_66', 'rows_2049_4096_5000')
LANES_G = (2, 4, 8, 16, 32, 64)


def lanes_lens(G):
  """Row lengths 0, 1, G - 1, G, G + 1 and 3 G + 2, forty of each, shuffled."""
  lens = [0, 1, G - 1, G, G + 1, 3 * G + 2] * 40
  order = _rng(8, G).permutation(len(lens))
  return [lens[i] for i in order]


# more rows than one pass of the lanes-per-row grid covers at any G: G = 2 puts 128 rows into each of at most GRID_CAP
# workgroups = 2^20 rows per pass
LANES_STRIDE_M = 2 ** 21
assert LANES_STRIDE_M > GRID_CAP * (256 // 2)


@functools.lru_cache(maxsize=None)
def lanes_stride_matrix(dtype):
  m = LANES_STRIDE_M
  rng = _rng(10)
  rows = np.unique(np.concatenate([[0, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, m - 1], rng.randint(0, m, size=600)]))
  lens = np.zeros(m, np.int64)
  lens[rows] = rng.choice([1, 2, 3, 5, 8, 13], size=rows.size)
  return csr_from_lens(lens, 500, dtype, 10)


def unreferenced(ncols):
  """Columns no entry of the matrices below refers to: the non-finite tests plant NaN / Inf at these positions of x."""
  return (0, ncols // 2, ncols - 1)


@functools.lru_cache(maxsize=None)
def matrix(family, name, dtype, ncols=6000):
  """The CSR matrix of a named row-length table; the columns unreferenced(ncols) are referenced by no entry."""
  lens = {'whole': planned_whole_lens, 'long': long_row_lens}[family]()[name] if family != 'lanes' else lanes_lens(int(name))
  return csr_from_lens(lens, ncols, dtype, len(name), avoid=unreferenced(ncols))


# ---------------------------------------------------------------------------------------------------- COO lists
COO_NNZ = (4095, 4096, 4097, 2 * 4096 + 1, 70001)
COO_RUNS = (1, 2, 5, 64, 257, 1000)
COO_SHAPE = (300, 400)


@functools.lru_cache(maxsize=None)
def coo_list(nnz, dtype, kind='runs', whole=False):
  """(rows, cols, vals) int32 / int32 / dtype.  'runs': duplicate runs of the lengths COO_RUNS (each cell's entries
  scattered through the list by a shuffle), at least 40 cells of >= 5 entries.  'one_cell': every entry in one cell.
  'distinct': no two entries share a cell."""
  rng = _rng(11, nnz, len(kind))
  nrows, ncols = COO_SHAPE
  if kind == 'one_cell':
    cell = np.full(nnz, 123 * ncols + 45, np.int64)
  elif kind == 'distinct':
    cell = rng.choice(nrows * ncols, size=nnz, replace=False).astype(np.int64)
  else:
    runs = [1000, 257, 257] + [64] * 6 + [5] * 40 + [2, 1]
    while sum(runs) + 1000 < nnz:
      runs.append(int(rng.choice(COO_RUNS)))
    while sum(runs) < nnz:
      runs.append(min(nnz - sum(runs), 2 if len(runs) % 2 else 1))
    assert sum(runs) == nnz
    cells = rng.choice(nrows * ncols, size=len(runs), replace=False).astype(np.int64)
    cell = np.repeat(cells, runs)[rng.permutation(nnz)]
  vals = (whole_values if whole else real_values)(nnz, dtype, 11, len(kind))
  return _freeze((cell // ncols).astype(np.int32), (cell % ncols).astype(np.int32), vals)


DROP_PATTERNS = ('every_third', 'block_256', 'all', 'first_and_last')


def dropped(rows, pattern):
  rows = np.array(rows)
  if pattern == 'every_third':
    rows[::3] = -1
  elif pattern == 'block_256':
    rows[1024:1280] = -1
  elif pattern == 'all':
    rows[:] = -1
  else:
    rows[0] = rows[-1] = -1
  return rows


# shapes on both sides of nrows * ncols + 1 = 2^8, 2^16, 2^24, 2^32, 2^40, 2^48, and 51 bits: (shape, radix passes of 8 bits)
KEY_WIDTH_SHAPES = (((15, 17), 1), ((16, 16), 2), ((255, 257), 2), ((256, 256), 3), ((2 ** 12 - 1, 2 ** 12 + 1), 3),
                    ((2 ** 12, 2 ** 12), 4), ((2 ** 16 - 1, 2 ** 16 + 1), 4), ((2 ** 16, 2 ** 16), 5),
                    ((2 ** 20 - 1, 2 ** 20 + 1), 5), ((2 ** 20, 2 ** 20), 6), ((2 ** 20, 2 ** 28 - 1), 6),
                    ((2 ** 20, 2 ** 28), 7), ((2 ** 20, 2 ** 31 - 1), 7))


def key_passes(shape):
  """8-bit radix passes sp_coo_to_csr runs: keys are below nrows * ncols, and the all-ones key of dropped entries
  must stay above every one of them."""
  span = int(shape[0]) * int(shape[1]) + 1
  nbits = 1
  while nbits < 64 and (1 << nbits) < span:
    nbits += 1
  return (nbits + 7) // 8


@functools.lru_cache(maxsize=None)
def key_width_list(shape, dtype):
  """About 2000 real-valued entries with duplicates: both corners of the shape (in runs of 5 and 7) and random cells."""
  nrows, ncols = shape
  rng = _rng(12, nrows, ncols & 0xffff)
  ncell = min(700, nrows * ncols)
  r = rng.randint(0, nrows, size=ncell).astype(np.int64)
  c = rng.randint(0, ncols, size=ncell).astype(np.int64)
  pick = rng.randint(0, ncell, size=2000)
  r = np.concatenate([r[pick], np.zeros(5, np.int64), np.full(7, nrows - 1, np.int64)])
  c = np.concatenate([c[pick], np.zeros(5, np.int64), np.full(7, ncols - 1, np.int64)])
  order = rng.permutation(r.size)
  return _freeze(r[order].astype(np.int32), c[order].astype(np.int32), real_values(r.size, dtype, 12, nrows))


# ---------------------------------------------------------------------------------------------------- n > 1
SPMM_N = (2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 259)
SPMM_LENS = (0, 1, 3, 4, 5, 8, 9, 40)
SPMM_K = 97


@functools.lru_cache(maxsize=None)
def spmm_matrix(dtype):
  """160 rows (more than one workgroup at every lane count) of the lengths SPMM_LENS -- around the unroll of 4 -- with
  empty first and last rows; the columns unreferenced(SPMM_K) hold no entry."""
  lens = list(SPMM_LENS) * 20
  order = _rng(13).permutation(len(lens))
  lens = [0] + [lens[i] for i in order][:-2] + [0]
  return csr_from_lens(lens, SPMM_K, dtype, 13, avoid=unreferenced(SPMM_K))


# ---------------------------------------------------------------------------------------------------- blocked kernel
BSP_S = 11264            # columns per slice of x


@functools.lru_cache(maxsize=None)
def band_matrix(m, k, nnz, avoid=()):
  """float32 [m, k] with nnz entries, site-local like PageRank's links: the entries of column c sit in rows around
  c * m / k, so that a row block draws its columns from one or two slices and the plan stages them.  Columns in
  `avoid` hold no entry."""
  allowed = np.setdiff1d(np.arange(k, dtype=np.int64), np.asarray(avoid, np.int64))
  per = -(-nnz // allowed.size)
  assert per <= 60
  offs = _rng(14, m, k).permutation(np.arange(-40, 41))[:per].astype(np.int64)     # distinct: no duplicate coordinates
  cols = np.tile(allowed, per)[:nnz]
  j = np.repeat(np.arange(per), allowed.size)[:nnz]
  rows = (cols * m // k + offs[j]) % m
  a = sps.coo_matrix((real_values(nnz, np.float32, 14, m, k), (rows, cols)), shape=(m, k)).tocsr()
  a.sort_indices()
  assert a.nnz == nnz and a.has_canonical_format
  a.indptr = a.indptr.astype(np.int64)
  _freeze(a.data, a.indices, a.indptr)
  return a


def staged_segments(plan_bytes):
  """(col_lo, width) of the staged segments in a plan of csrc/spmv_blocked.hip (header: valid, rows per block, blocks,
  slice width, slices, nnz, m, k; then the segment counts and 64 segments {col_lo, width, count, staged} per block)."""
  p = np.asarray(plan_bytes, np.uint8)
  header = p[:64].view(np.int64)
  nb = int(header[2])
  al = lambda n: (n + 255) & ~255        # noqa: E731
  nseg = p[256:256 + nb * 4].view(np.int32)
  seg_off = 256 + al(nb * 4)
  segs = p[seg_off:seg_off + nb * 64 * 16].view(np.int32).reshape(nb, 64, 4)
  out = set()
  for b in range(nb):
    for s in segs[b, :nseg[b]]:
      if s[3]:
        out.add((int(s[0]), int(s[1])))
  return sorted(out)
