"""Cases, oracle, ordered restatement and derived bounds of the cosine top-k kernels (sp_item_topk / sp_item_topk_merge,
include/spartan_hip_cf.h) and of the item recommender (spartan_amd/examples/cf).  Shared by the CPU and the GPU tests;
nothing here touches a device.

THE BOUND OF A SIMILARITY.  u = eps / 2 is the unit roundoff of the operands' dtype T; the norms tnorm[j], snorm[i] are
taken as given inputs.  For target column j and source column i over `users` users, every operation rounded once
(relative error <= u), to first order in u:
    p_u = t[u][j] * s[u][i]                 u each
    dot = (((0 + p_0) + p_1) + ...)         the first addition is exact; a product passes through at most users - 1
                                            additions that round: |dot - exact| <= (u + (users - 1) u) S = users u S,
                                            S = sum_u |t[u][j] s[u][i]|
    den = tnorm[j] * snorm[i]               u
    sim = dot / den                         u (IEEE division), and den's u: 2 u |sim|, with |sim| <= S / den
Together |sim - exact| <= c u S / (tnorm[j] snorm[i]) with c = users + 2 (`users` products-and-additions, the product of
norms, the division); gamma = c u / (1 - c u) takes care of the higher orders.  Any other order of the additions (the
reference's BLAS or sparse product) obeys the same bound.  The bound assumes no product underflows and nothing
overflows; the random cases keep their entries of order 1.  Where den == 0 the quotient is 0 / 0 = NaN and nan_to_num
makes it exactly +0 on both sides: bound 0.  nan_to_num's other branches (infinities) are pinned by the byte-for-byte
tests on special values, not by this bound.

THE DRIVER'S BOUND adds the norms' own rounding.  norm = sqrt(sum_u r_u^2): the squares are u each, all summands are
>= 0 so the users - 1 rounding additions add u each to the relative error: users u; the square root halves that and
adds u: (users / 2 + 1) u per norm, (users + 2) u for the two, relative to |sim|:
    |sim - exact| <= gamma(users + 2) S / (|t| |s|) + gamma(users + 2) |sim|
with |t|, |s| now the exact norms.  A float64 reference run obeys it with float64's u; ours against the reference's
recording is within the sum of the two.

TIES AND THE CUT.  The kernel's order is (similarity descending, index ascending).  Against the oracle an index SET is
asserted for a row only where the oracle's k-th and (k + 1)-th largest similarities differ by more than twice the
row's largest bound (otherwise rounding may legitimately swap them: such a row is compared by values only); the
ordered LIST where that holds for every neighbouring pair of the first k + 1.  With 0 or 1 users every similarity is
0 or +-1 and every row ties by construction: those cases are compared by values only and are left out of the count
of "values only" rows, which must stay below 5 % of all others (the seeds below were chosen on the CPU so that the
oracle alone satisfies it).  The order under ties is pinned by the byte-for-byte tests instead."""
import functools

import numpy as np

LD = np.longdouble
TILE, CHUNK = 64, 16                          # targets / sources per block and users per chunk of cf_scan_kernel
MAX_K = 128                                   # SP_CF_MAX_K
ITEMS = (1, 2, 3, 63, 64, 65, 130, 257)       # both sides of the 64-item tile, more than one block, odd sizes
USERS = (0, 1, 15, 16, 17, 33, 200)           # both sides of the 16-user chunk
KS = (1, 5, 10, 64, 128)
DTYPES = (np.float32, np.float64)
VALUES_ONLY_SHARE = 0.05

GOLDEN_USERS, GOLDEN_ITEMS, GOLDEN_K, GOLDEN_ZERO_ITEM, GOLDEN_SEED = 40, 24, 5, 7, 20261020


def ranges_of(m, ns, k, splits):
  """Into how many ranges of columns sp_item_topk cuts the sources (cf_ranges of csrc/cf.hip, stated in the header)."""
  if ns <= 0:
    return 1
  if splits >= 1:
    return min(splits, ns)
  r = max(1, min(-(-512 // -(-m // TILE)) if m > 0 else 1, -(-ns // max(4 * k, TILE)), 64))
  if r == 1:
    return 1
  passes = -(-(-(-ns // r)) // TILE)
  return -(-ns // (TILE * passes))


def unit_roundoff(dtype):
  return float(np.finfo(np.dtype(dtype)).eps) / 2


def gamma(c, dtype):
  cu = c * unit_roundoff(dtype)
  return cu / (1 - cu)


def share(err, bound):
  """The largest err / bound (0 / 0 counts as 0; an error above a zero bound as inf)."""
  err, bound = np.asarray(err, LD), np.asarray(bound, LD)
  with np.errstate(all='ignore'):
    q = np.where(err == 0, LD(0), err / bound)
  return float(np.max(q)) if q.size else 0.0


def norms_of(table):
  """The columns' norms in the table's dtype, as a caller of the kernel computes them."""
  table = np.asarray(table)
  with np.errstate(all='ignore'):
    return np.sqrt((table * table).sum(axis=0)).astype(table.dtype)


@functools.lru_cache(maxsize=None)
def _table_case(users, items, dtype, seed):
  dt = np.dtype(dtype)
  rng = np.random.default_rng(100003 * users + 101 * items + seed)
  table = rng.standard_normal((users, items)).astype(dt)
  norms = norms_of(table)
  table.setflags(write=False)
  norms.setflags(write=False)
  return table, norms


def table_case(users, items, dtype, seed=0):
  """(table [users, items], norms [items]) in `dtype`, read-only: standard normal ratings."""
  return _table_case(int(users), int(items), np.dtype(dtype).name, int(seed))


def oracle(targets, tnorm, sources, snorm):
  """(sim [m, ns], bound [m, ns]) in longdouble: the exact similarities of the operands as given, nan_to_num applied
  (0 where the product of norms is 0), and the bound of the module docstring in the operands' dtype."""
  dt = np.asarray(targets).dtype
  t, s = np.asarray(targets, LD), np.asarray(sources, LD)
  users = t.shape[0]
  dot = np.zeros((t.shape[1], s.shape[1]), LD)
  mag = np.zeros((t.shape[1], s.shape[1]), LD)
  for u in range(users):
    p = t[u][:, None] * s[u][None, :]
    dot += p
    mag += np.abs(p)
  den = np.asarray(tnorm, LD)[:, None] * np.asarray(snorm, LD)[None, :]
  with np.errstate(all='ignore'):
    sim = np.where(den == 0, LD(0), dot / den)
    bound = np.where(den == 0, LD(0), LD(gamma(users + 2, dt)) * mag / den)
  assert np.isfinite(sim).all() and np.isfinite(bound).all()
  return sim, bound


def restated_similarities(targets, tnorm, sources, snorm):
  """[m, ns] as the header states them, written out target by target: one accumulator per pair that starts at 0 and
  takes t[u][j] * s[u][i] for u = 0, 1, ... in turn, one product of norms, one division, nan_to_num."""
  targets, sources = np.asarray(targets), np.asarray(sources)
  dt = targets.dtype
  users, m = targets.shape
  ns = sources.shape[1]
  sim = np.empty((m, ns), dt)
  with np.errstate(all='ignore'):
    for j in range(m):
      acc = np.zeros(ns, dt)
      for u in range(users):
        acc = acc + targets[u, j] * sources[u]
      sim[j] = np.nan_to_num(acc / (tnorm[j] * snorm))
      assert acc.dtype == dt
  return sim


def restated_selection(all_sim, k, index_offset=0):
  """(sim [m, k], idx [m, k]): per row of the [m, ns] similarities the k best by (similarity descending, index
  ascending), idx = index_offset + column, padded with -inf / -1."""
  m, ns = all_sim.shape
  sim = np.full((m, k), -np.inf, all_sim.dtype)
  idx = np.full((m, k), -1, np.int64)
  for j in range(m):
    row = all_sim[j]
    best = sorted(range(ns), key=lambda i: (-row[i], i))[:k]
    sim[j, :len(best)] = row[best]
    idx[j, :len(best)] = np.asarray(best, np.int64) + index_offset
  return sim, idx


def restatement(targets, tnorm, sources, snorm, k, index_offset=0):
  """restated_selection of restated_similarities.  Tests compare BYTES against it."""
  return restated_selection(restated_similarities(targets, tnorm, sources, snorm), k, index_offset)


@functools.lru_cache(maxsize=None)
def case_similarities(users, items, dtype, seed=0):
  """restated_similarities of table_case(users, items, dtype, seed) against itself; computed once, read-only."""
  table, norms = table_case(users, items, dtype, seed)
  sim = restated_similarities(table, norms, table, norms)
  sim.setflags(write=False)
  return sim


@functools.lru_cache(maxsize=None)
def case_oracle(users, items, dtype, seed=0):
  """oracle of table_case(users, items, dtype, seed) against itself; computed once."""
  table, norms = table_case(users, items, dtype, seed)
  return oracle(table, norms, table, norms)


def restate_merge(cand_sim, cand_idx, k):
  """(sim [m, k], idx [m, k]): per row the k best candidates by (similarity descending, index ascending); candidates
  with a negative index or a NaN similarity are ignored; padded with -inf / -1."""
  cand_sim, cand_idx = np.asarray(cand_sim), np.asarray(cand_idx)
  m = cand_sim.shape[0]
  sim = np.full((m, k), -np.inf, cand_sim.dtype)
  idx = np.full((m, k), -1, np.int64)
  for j in range(m):
    live = [c for c in range(cand_sim.shape[1]) if cand_idx[j, c] >= 0 and cand_sim[j, c] == cand_sim[j, c]]
    best = sorted(live, key=lambda c: (-cand_sim[j, c], cand_idx[j, c]))[:k]
    sim[j, :len(best)] = cand_sim[j, best]
    idx[j, :len(best)] = cand_idx[j, best]
  return sim, idx


def check_topk(got_sim, got_idx, exact, bound, k, index_offset=0, label=''):
  """Asserts (sim, idx) [m, k] against the oracle's (exact, bound) [m, ns]: every value within the bound of its own
  pair, the e-th value within the row's largest bound of the oracle's e-th best, padding exactly where ns < k, the
  index set / list where the cut / every gap is clear (module docstring).  Returns (largest share of a bound, rows left
  to values only, rows)."""
  got_sim, got_idx = np.asarray(got_sim), np.asarray(got_idx)
  m, ns = exact.shape
  kept = min(k, ns)
  assert got_sim.shape == (m, k) and got_idx.shape == (m, k) and got_idx.dtype == np.int64, (got_sim.shape, got_idx.shape)
  assert (got_idx[:, kept:] == -1).all() and np.isneginf(got_sim[:, kept:]).all(), label
  worst, values_only = 0.0, 0
  for j in range(m):
    cols = got_idx[j, :kept] - index_offset
    assert ((cols >= 0) & (cols < ns)).all() and len(set(cols.tolist())) == kept, (label, j, cols)
    worst = max(worst, share(np.abs(np.asarray(got_sim[j, :kept], LD) - exact[j, cols]), bound[j, cols]))
    order = sorted(range(ns), key=lambda i: (-exact[j, i], i))
    ranked = exact[j, order]
    row_bound = bound[j].max() if ns else LD(0)
    worst = max(worst, share(np.abs(np.asarray(got_sim[j, :kept], LD) - ranked[:kept]), np.full(kept, row_bound)))
    gaps = ranked[:kept] - np.append(ranked[1:kept], ranked[kept] if ns > kept else -np.inf)
    if gaps[-1] > 2 * row_bound:
      assert set(cols.tolist()) == set(order[:kept]), (label, j)
      if (gaps > 2 * row_bound).all():
        assert cols.tolist() == order[:kept], (label, j)
    else:
      values_only += 1
  return worst, values_only, m


# ---- the recommender's golden ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_input():
  """The rating table tests/golden/item_recommender_w4.npz is recorded on: 40 users x 24 items, float64, about 30 %
  filled with ratings uniform in -5 .. 5 (negative ones included), item 7 rated by nobody; read-only."""
  rng = np.random.default_rng(GOLDEN_SEED)
  filled = rng.random((GOLDEN_USERS, GOLDEN_ITEMS)) < 0.3
  table = np.where(filled, rng.uniform(-5.0, 5.0, (GOLDEN_USERS, GOLDEN_ITEMS)), 0.0)
  table[:, GOLDEN_ZERO_ITEM] = 0.0
  assert table.dtype == np.float64 and (table < 0).any()
  table.setflags(write=False)
  return table


def driver_oracle(table, dtype):
  """(sim [N, N], bound [N, N]) in longdouble for the table rounded to `dtype`: the exact similarities with exact
  norms and the driver's bound of the module docstring in `dtype`."""
  t = np.asarray(np.asarray(table).astype(dtype), LD)
  users = t.shape[0]
  norm = np.sqrt((t * t).sum(axis=0))
  dot = t.T.dot(t)
  mag = np.abs(t).T.dot(np.abs(t))
  den = norm[:, None] * norm[None, :]
  with np.errstate(all='ignore'):
    sim = np.where(den == 0, LD(0), dot / den)
    g = LD(gamma(users + 2, dtype))
    bound = np.where(den == 0, LD(0), g * mag / den + g * np.abs(sim))
  return sim, bound


def rows_by_order(sim, idx):
  """Rows re-sorted by (value descending, index ascending)."""
  sim, idx = np.asarray(sim), np.asarray(idx, np.int64)
  order = np.lexsort((idx, -sim), axis=1)
  return np.take_along_axis(sim, order, axis=1), np.take_along_axis(idx, order, axis=1)


def golden_gaps_are_clear(table, k, extra=1.0):
  """True if in every row but the all-zero item's the oracle's k-th and (k + 1)-th largest similarities differ by more
  than twice `extra` times the row's largest float64 driver bound."""
  sim, bound = driver_oracle(table, np.float64)
  for j in range(sim.shape[0]):
    if j == GOLDEN_ZERO_ITEM:
      continue
    ranked = np.sort(sim[j])[::-1]
    if not ranked[k - 1] - ranked[k] > 2 * extra * bound[j].max():
      return False
  return True
