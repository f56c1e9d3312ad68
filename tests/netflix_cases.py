"""Cases, the restated sequence and the yardstick for sp_sgd_mf (include/spartan_hip_mf.h), examples/_netflix.py and
the Netflix SGD driver.  No GPU, no backend: NumPy only.

  restated(...)    the sequence one entry at a time in tile order, scalar by scalar in the arrays' dtype T: the lane sums
                   in ascending order, the balanced tree, one rounding per operation.  NO schedule.  Written apart from
                   examples/_netflix.sgd_numpy (which works on rows) so that the two check each other; the kernel and
                   sp_sgd_mf_host are held to it byte for byte.  dot='plain' replaces the inner product by the plain
                   left-to-right sum of the reference's compiled loop.
  yardstick(...)   the same sequence in float64 NumPy with plain sums, on the inputs as they are.
  epochs(body, ...)  whole epochs over the blocks of a grid, stratum by stratum, with `body` as the tile pass.

The accuracy rule (svm's).  tests/golden/netflix_w4.npz holds the reference's own run in float32 (U and M after epochs 1
and 2, the strata it drew).  e_ref is the largest absolute distance of a recorded array to the float64 yardstick of the
same sequence in the same strata; a float32 run of ours must lie within 8 e_ref of that yardstick and a float64 run
within 8 e_ref / 2^29 (2^29: the ratio of the unit roundoffs).  Ours and the reference's differ in the order of a
20-term sum only, and the error is dominated by the update's rounding, not by the dot.  What the golden gives (largest
distance to the yardstick over e_ref, in float64 over e_ref / 2^29; the tests print every ratio before they assert):
                                              U epoch 1   M epoch 1   U epoch 2   M epoch 2      (e_ref = 2.25e-7)
    float32  restated = sgd_numpy = sp_sgd_mf_host,
             NumpyBackend driver, HIP driver     0.57        0.30        1.00        0.59
    float64  the same                            0.00        0.13        0.13        0.13
(one row per dtype: every path of ours gives the stated order's bytes.)  The largest is 1.00 of the 8 allowed; the
factors moved by 5.9e-4 over the two epochs, 328 times the limit 8 e_ref.  With the plain left-to-right dot in the place
of the stated one, restated gives the reference's recorded bytes.

NaN.  "Byte for byte" holds for every value that is not a NaN: the sign and payload of a NaN that an operation makes
differ between processors, so `same` compares NaN by position and everything else by its bytes.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'netflix_w4.npz')

# the golden recipe
USERS, MOVIES, GRID, RANK, RATINGS, EPOCHS, WORKERS = 52, 400, 4, 20, 1500, 2, 4
FACTOR = 8.0
F32_OVER_F64 = 2.0 ** 29
LR = float(np.float32(1e-5))

# the device ranks: both sides of every lanes-per-rating boundary (8 lanes to 16, 16 lanes to 64) and of the limit
RANKS = (1, 7, 16, 17, 20, 64, 65, 500, 512)


def same(got, want):
  """Equal byte for byte, a NaN standing for any NaN."""
  got, want = np.asarray(got), np.asarray(want)
  if got.shape != want.shape or got.dtype != want.dtype:
    return False
  gn, wn = np.isnan(got), np.isnan(want)
  return bool((gn == wn).all()) and np.where(gn, 0, got).tobytes() == np.where(wn, 0, want).tobytes()


def lanes_of(f):
  return 8 if f <= 16 else (16 if f <= 64 else 64)


def stated_dot(p, q):
  """dot(p, q) in the header's order, scalar by scalar in the vectors' dtype."""
  f, lanes = len(p), lanes_of(len(p))
  zero = p.dtype.type(0)
  sums = []
  for lane in range(lanes):
    acc = zero
    for a, b in zip(p[lane::lanes], q[lane::lanes]):
      acc = acc + a * b
    sums.append(acc)
  s = lanes // 2
  while s >= 1:
    sums = [sums[i] + sums[i + s] for i in range(s)]
    s //= 2
  return sums[0]


def plain_dot(p, q):
  """The reference's compiled loop: guess = guess + u[k] * m[k], k ascending."""
  acc = p.dtype.type(0)
  for a, b in zip(p, q):
    acc = acc + a * b
  return acc


def restated(indptr, indices, vals, u, m, lr=LR, dot='stated', order=None):
  """(U', M', abs_err) of one pass in tile order (or in `order`, a list of entry indices), every operation in the
  arrays' dtype; the operands are not written."""
  dt = u.dtype
  f = u.shape[1]
  lr = dt.type(lr)
  inner = stated_dot if dot == 'stated' else plain_dot
  u, m = np.array(u), np.array(m)
  rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
  abs_err = np.zeros(len(indices), dt)
  with np.errstate(all='ignore'):
    for e in (range(len(indices)) if order is None else order):
      i, j = int(rows[e]), int(indices[e])
      d = vals[e] - inner(u[i], m[j])
      abs_err[e] = abs(d)
      for k in range(f):
        u[i, k] = u[i, k] + (u[i, k] * d) * lr
        m[j, k] = m[j, k] + (m[j, k] * d) * lr
  assert u.dtype == dt and m.dtype == dt and abs_err.dtype == dt
  return u, m, abs_err


def yardstick(indptr, indices, vals, u, m, lr=LR):
  """The same sequence in float64 with NumPy's sums: (U', M') as float64 arrays.  (lr is rounded to the operands' dtype
  first: that rounding is part of the contract, not of the error.)"""
  lr = np.float64(np.asarray(u).dtype.type(lr)) if np.asarray(u).dtype != np.float64 else np.float64(lr)
  u, m = np.array(u, np.float64), np.array(m, np.float64)
  vals = np.asarray(vals, np.float64)
  rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
  for e in range(len(indices)):
    i, j = int(rows[e]), int(indices[e])
    d = vals[e] - np.dot(u[i], m[j])
    u[i] = u[i] + (u[i] * d) * lr
    m[j] = m[j] + (m[j] * d) * lr
  return u, m


def csr(shape, rows, cols, vals, dtype):
  """Canonical CSR (int64 indptr, int32 indices ascending inside a row, values) of distinct coordinates."""
  rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
  assert len(set(zip(rows.tolist(), cols.tolist()))) == len(rows)
  order = np.lexsort((cols, rows))
  indptr = np.zeros(shape[0] + 1, np.int64)
  np.add.at(indptr, rows + 1, 1)
  return np.cumsum(indptr), cols[order].astype(np.int32), np.asarray(vals, dtype)[order]


def factors(m, n, f, dtype, seed=0, ld_extra=0):
  """(U [m, f], M [n, f]) in `dtype`, of order 1 / sqrt(f) so that a dot is of order 1 and d of order the rating; with
  ld_extra the arrays are row views of arrays ld_extra columns wider (the rest holds 7)."""
  rng = np.random.RandomState(100 + seed)
  out = []
  for rows in (m, n):
    wide = np.full((rows, f + ld_extra), 7.0, dtype)
    wide[:, :f] = (rng.rand(rows, f) + 0.5) / np.sqrt(f)
    out.append(wide[:, :f])
  return out


def random_tile(m, n, nnz, dtype, seed=0):
  """(indptr, indices, vals): about nnz distinct cells of an m x n tile, ratings 1 .. 5."""
  rng = np.random.RandomState(7 + seed)
  cells = np.unique(rng.randint(0, m * n, nnz))
  return csr((m, n), cells // n, cells % n, rng.randint(1, 6, len(cells)), dtype)


def pairs_tile(p, dtype, shift=0, tail=0):
  """(shape, (indptr, indices, vals)) of a tile with p disjoint (row, column) pairs (i, i): ONE level of width p.
  shift = 1 adds the same pairs shifted by one column, (i, i + 1).  In the tile's stored order (i, i + 1) comes before
  (i + 1, i + 1) in column i + 1, so this is one dependent chain of 2 p levels of width 1, not a second wide level.
  shift = p adds (i, p + i) and (p + i, i) instead: each follows (i, i) in its row or in its column and shares nothing
  else, so they form a second level, 2 p wide, that depends on the first.  `tail` adds that many entries
  (2 p + t, 2 p): a chain of narrow levels in a column of their own."""
  assert shift in (0, 1, p)
  rows, cols = list(range(p)), list(range(p))
  if shift == 1:
    rows += list(range(p))
    cols += [i + 1 for i in range(p)]
  elif shift == p:
    rows += list(range(p)) + [p + i for i in range(p)]
    cols += [p + i for i in range(p)] + list(range(p))
  for t in range(tail):
    rows.append(2 * p + t)
    cols.append(2 * p)
  rng = np.random.RandomState(p + tail)
  shape = (2 * p + tail, 2 * p + 1)
  return shape, csr(shape, rows, cols, rng.randint(1, 6, len(rows)), dtype)


def tree_tile(wide, dtype, tail=3):
  """A tile whose schedule goes narrow, wide, narrow.  A level can be at most twice as wide as the one before it (an
  entry has one successor in its row and one in its column), so the narrow levels double -- 1, 2, 4, ... entries: the
  entry (i, j) of one level is followed by (i, a new column) and (a new row, j) in the next -- until a level holds at
  least `wide` entries; after it a chain of `tail` single entries continues one row.  Returns (shape, (indptr, indices,
  vals), widths of the levels)."""
  rows, cols = [0], [0]
  frontier, next_row, next_col, widths = [(0, 0)], 1, 1, [1]
  while len(frontier) < wide:
    grown = []
    for i, j in frontier:
      grown += [(i, next_col), (next_row, j)]
      next_row, next_col = next_row + 1, next_col + 1
    frontier = grown
    rows += [i for i, _ in grown]
    cols += [j for _, j in grown]
    widths.append(len(grown))
  i = frontier[0][0]
  for _ in range(tail):
    rows.append(i)
    cols.append(next_col)
    next_col += 1
    widths.append(1)
  rng = np.random.RandomState(len(rows))
  shape = (next_row, next_col)
  return shape, csr(shape, rows, cols, rng.randint(1, 6, len(rows)), dtype), widths


def golden_input():
  """(rows, cols, vals float32) of about 1500 distinct ratings 1 .. 5 on 52 users x 400 movies, and U0 [52, 20],
  M0 [400, 20] float32: the recipe of the golden."""
  rng = np.random.RandomState(20150708)
  cells = np.unique(rng.randint(0, USERS * MOVIES, RATINGS))
  rows, cols = cells // MOVIES, cells % MOVIES
  vals = rng.randint(1, 6, len(cells)).astype(np.float32)
  u0 = ((rng.rand(USERS, RANK) + 0.5) / np.sqrt(RANK)).astype(np.float32)
  m0 = ((rng.rand(MOVIES, RANK) + 0.5) / np.sqrt(RANK)).astype(np.float32)
  return rows, cols, vals, u0, m0


def grid_cuts(n, parts):
  """The tile boundaries of one axis: blocks of divup(n, parts)."""
  step = -(-n // parts)
  return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def block(rows, cols, vals, rcut, ccut, dtype):
  """The block [rcut) x [ccut) of a COO list as canonical CSR with local coordinates."""
  keep = (rows >= rcut[0]) & (rows < rcut[1]) & (cols >= ccut[0]) & (cols < ccut[1])
  return csr((rcut[1] - rcut[0], ccut[1] - ccut[0]), rows[keep] - rcut[0], cols[keep] - ccut[0], vals[keep], dtype)


def default_strata(gr, gc):
  g = max(gr, gc)
  return [[(i, j) for i in range(gr) for j in range(gc) if (j - i) % g == s] for s in range(g)]


def epochs(body, rows, cols, vals, u0, m0, strata, n_epochs=EPOCHS, dtype=np.float32, lr=LR):
  """[(U, M) after every epoch] with `body(indptr, indices, vals, u, m, lr) -> (u', m', ...)` as the pass over a block;
  `strata` holds one stratification per epoch (the reference draws a new one for every epoch): lists of lists of block
  coordinates (bi, bj) of the GRID x GRID grid, taken in the order given."""
  dt = np.dtype(dtype)
  wide = body is yardstick
  u = np.array(u0, np.float64 if wide else dt)
  m = np.array(m0, np.float64 if wide else dt)
  rcuts, ccuts = grid_cuts(u.shape[0], GRID), grid_cuts(m.shape[0], GRID)
  out = []
  assert len(strata) == n_epochs
  for t in range(n_epochs):
    for stratum in strata[t]:
      for bi, bj in stratum:
        (r0, r1), (c0, c1) = rcuts[bi], ccuts[bj]
        indptr, indices, bv = block(rows, cols, vals, rcuts[bi], ccuts[bj], dt)
        if wide:
          un, mn = _yardstick_wide(indptr, indices, bv, u[r0:r1], m[c0:c1], dt.type(lr))
        else:
          un, mn = body(indptr, indices, bv, u[r0:r1], m[c0:c1], lr)[:2]
        u[r0:r1], m[c0:c1] = un, mn
    out.append((u.copy(), m.copy()))
  return out


def _yardstick_wide(indptr, indices, vals, u, m, lr):
  """yardstick on float64 factors that are not rounded between blocks (lr already rounded to the run's dtype)."""
  u, m = np.array(u), np.array(m)
  lr = np.float64(lr)
  vals = np.asarray(vals, np.float64)
  rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
  for e in range(len(indices)):
    i, j = int(rows[e]), int(indices[e])
    d = vals[e] - np.dot(u[i], m[j])
    u[i] = u[i] + (u[i] * d) * lr
    m[j] = m[j] + (m[j] * d) * lr
  return u, m


_cache = {}


def golden():
  if 'golden' not in _cache:
    _cache['golden'] = dict(np.load(GOLDEN))
  return _cache['golden']


def golden_strata():
  """The strata the reference drew, one stratification per epoch, as lists of lists of block coordinates (bi, bj) in
  its order.  (strata_blocks [16 EPOCHS, 2] lists the blocks, strata_sizes the blocks per stratum, strata_counts the
  strata per epoch.)"""
  g = golden()
  flat, sizes, counts = g['strata_blocks'], g['strata_sizes'], g['strata_counts']
  out, at, s = [], 0, 0
  for c in counts:
    epoch = []
    for n in sizes[s:s + int(c)]:
      epoch.append([(int(a), int(b)) for a, b in flat[at:at + int(n)]])
      at += int(n)
    s += int(c)
    out.append(epoch)
  return out


def golden_yardstick(dtype=np.float32):
  """[(U, M) after epochs 1, 2] of the float64 yardstick in the golden's strata (inputs and lr rounded to `dtype`)."""
  key = ('yardstick', np.dtype(dtype).name)
  if key not in _cache:
    rows, cols, vals, u0, m0 = golden_input()
    _cache[key] = epochs(yardstick, rows, cols, vals, u0, m0, golden_strata(), dtype=dtype)
  return _cache[key]


def e_ref():
  """The largest absolute distance of the golden's recorded U and M (after either epoch) to the float64 yardstick."""
  g, want = golden(), golden_yardstick(np.float32)
  return max(float(np.abs(np.asarray(g[k % (t + 1)], np.float64) - want[t][w]).max())
             for t in range(EPOCHS) for w, k in ((0, 'U_%d'), (1, 'M_%d')))


def check_accuracy(got, dtype, label):
  """`got` = [(U, M) after epochs 1, 2] of a run of ours in `dtype` on the golden input in the golden's strata: prints
  every ratio to e_ref (to e_ref / 2^29 in float64), then asserts the rule.  Returns the largest ratio."""
  dt = np.dtype(dtype)
  want, ref = golden_yardstick(dt), e_ref()
  assert ref > 0
  limit = ref if dt == np.float32 else ref / F32_OVER_F64
  worst = 0.0
  for t in range(EPOCHS):
    for w, name in ((0, 'U'), (1, 'M')):
      err = float(np.abs(np.asarray(got[t][w], np.float64) - want[t][w]).max())
      worst = max(worst, err / limit)
      print('%s %s %s after epoch %d: max abs distance to the yardstick %.3g, e_ref %.3g, ratio %.3g (limit %g)'
            % (label, dt.name, name, t + 1, err, ref, err / limit, FACTOR))
  assert worst <= FACTOR, (label, worst)
  return worst


def dense_tile(k, dtype):
  """A dense k x k block: the levels are the anti-diagonals, 2 k - 1 of them."""
  rng = np.random.RandomState(k)
  return csr((k, k), np.repeat(np.arange(k), k), np.tile(np.arange(k), k), rng.randint(1, 6, k * k), dtype)


def special_tile(dtype):
  """(shape, csr, {name: entry index}) of 12 x 80: rows 0 .. 5 hold about 120 ratings in columns 0 .. 39, of which one
  is NaN and one +inf; rows 6 .. 11 hold about 120 in columns 40 .. 79, of which one is 0.  The two halves share neither
  rows nor columns: what the NaN poisons stays in the first."""
  ap, ai, av = random_tile(6, 40, 130, dtype, seed=3)
  bp, bi, bv = random_tile(6, 40, 130, dtype, seed=4)
  indptr = np.concatenate([ap, ap[-1] + bp[1:]])
  indices = np.concatenate([ai, bi + 40]).astype(np.int32)
  vals = np.concatenate([av, bv])
  marks = {'nan': 17, 'inf': 60, 'zero': len(ai) + 50}
  vals[marks['nan']], vals[marks['inf']], vals[marks['zero']] = np.nan, np.inf, 0.0
  return (12, 80), (indptr, indices, vals), marks


def cases(dtype, wide):
  """{name: (shape, (indptr, indices, vals))}: the structures of the device tests, `wide` being SP_MF_WIDE."""
  p = wide + 5
  out = {
      'empty': ((5, 7), (np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype))),
      'one row': ((1, 50), random_tile(1, 50, 40, dtype)),
      'one column': ((50, 1), random_tile(50, 1, 40, dtype)),
      'dense 8 x 8': ((8, 8), dense_tile(8, dtype)),
      '13 x 1250': ((13, 1250), random_tile(13, 1250, 1000, dtype)),
      'pairs': pairs_tile(p, dtype),
      'pairs shifted by one column': pairs_tile(p, dtype, shift=1),
      'pairs and their successors': pairs_tile(p, dtype, shift=p, tail=3),
      'narrow wide narrow': tree_tile(wide, dtype)[:2],
      'special values': special_tile(dtype)[:2],
  }
  return out
