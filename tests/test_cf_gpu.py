"""sp_item_topk / sp_item_topk_merge (csrc/cf.hip) through HipBackend.item_topk / item_topk_merge and the launchers,
against the oracle, the derived bound and the ordered restatement of tests/cf_cases.py.

Items N = 1, 2, 3, 63, 64, 65, 130, 257 and users = 0, 1, 15, 16, 17, 33, 200, for the tile that was built
(include/spartan_hip_cf.h): a workgroup owns 64 targets and takes the sources 64 at a time in chunks of 16 users, so N
sits on both sides of 64 and spans more than one block, and the users sit on both sides of 16 and span more than one
chunk.  k = 1, 5, 10, 64, 128, both dtypes.  Nothing is larger.  Measured shares of the bound are printed before each
assertion (pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, devarray, kernels
from tests import cf_cases as cc

pytestmark = pytest.mark.gpu
IDS = dict(ids=lambda d: np.dtype(d).name)


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _dev(be, a):
  return be.from_numpy(np.ascontiguousarray(a))


def _topk(be, targets, tnorm, sources, snorm, k, **kw):
  sim, idx = be.item_topk(_dev(be, targets), _dev(be, tnorm), _dev(be, sources), _dev(be, snorm), k, **kw)
  return sim.numpy(), idx.numpy()


def _same(a, b):
  return a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype == np.int64 and a[0].tobytes() == b[0].tobytes() \
      and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize('dtype', cc.DTYPES, **IDS)
def test_every_value_meets_the_bound_and_equals_the_restatement(be, dtype):
  worst, unclear, rows = 0.0, 0, 0
  for users in cc.USERS:
    for items in cc.ITEMS:
      table, norms = cc.table_case(users, items, dtype)
      exact, bound = cc.case_oracle(users, items, dtype)
      stated = cc.case_similarities(users, items, dtype)
      d_table, d_norms = _dev(be, table), _dev(be, norms)
      for k in cc.KS:
        label = 'hip users=%d items=%d k=%d %s' % (users, items, k, np.dtype(dtype).name)
        before = be.launches
        sim, idx = be.item_topk(d_table, d_norms, d_table, d_norms, k)
        assert be.launches - before == (1 if cc.ranges_of(items, items, k, 0) == 1 else 2), label   # (257 items: two ranges)
        got = sim.numpy(), idx.numpy()
        assert got[0].dtype == np.dtype(dtype) and got[0].shape == (items, k), label
        w, v, m = cc.check_topk(got[0], got[1], exact, bound, k, label=label)
        worst = max(worst, w)
        if users >= 2:
          unclear, rows = unclear + v, rows + m
        assert _same(got, cc.restated_selection(stated, k)), label
      again = be.item_topk(d_table, d_norms, d_table, d_norms, cc.KS[-1])
      assert _same((again[0].numpy(), again[1].numpy()), got), (users, items)          # a repeated call: the same bytes
  print('item_topk hip %s: at %.3g of the bound; %d of %d rows by values only' % (np.dtype(dtype).name, worst, unclear, rows))
  assert worst <= 1.0
  assert unclear <= cc.VALUES_ONLY_SHARE * rows, (unclear, rows)


@pytest.mark.parametrize('dtype', cc.DTYPES, **IDS)
def test_splits_give_the_same_bytes(be, dtype):
  for users, items in ((33, 257), (200, 130), (17, 65), (16, 3)):
    table, norms = cc.table_case(users, items, dtype)
    for k in (1, 10, 128):
      want = cc.restated_selection(cc.case_similarities(users, items, dtype), k)
      for splits in (0, 1, 2, 3, 64):
        before = be.launches
        got = _topk(be, table, norms, table, norms, k, splits=splits)
        assert be.launches - before == (1 if cc.ranges_of(items, items, k, splits) == 1 else 2), (items, splits)   # the scan, and the merge
        assert _same(got, want), (users, items, k, splits)


@pytest.mark.parametrize('dtype', cc.DTYPES, **IDS)
def test_a_band_of_targets_gives_the_bytes_of_the_whole(be, dtype):
  users, items, k = 33, 257, 10
  table, norms = cc.table_case(users, items, dtype)
  whole = _topk(be, table, norms, table, norms, k)
  d_table, d_norms = _dev(be, table), _dev(be, norms)
  for lo in (1, 63, 64, 65):
    for m in (1, 64, 70):
      # the band as a column range of the table itself (ldt == lds == the table's row stride) ...
      view = be.item_topk(d_table[:, lo:lo + m], d_norms[lo:lo + m], d_table, d_norms, k, splits=lo % 3)
      assert _same((view[0].numpy(), view[1].numpy()), (whole[0][lo:lo + m], whole[1][lo:lo + m])), (lo, m)
      # ... and as a contiguous copy (ldt != lds)
      copy = _topk(be, table[:, lo:lo + m], norms[lo:lo + m], table, norms, k)
      assert _same(copy, (whole[0][lo:lo + m], whole[1][lo:lo + m])), (lo, m)


@pytest.mark.parametrize('dtype', cc.DTYPES, **IDS)
def test_strided_operands_give_the_bytes_of_contiguous_copies(be, dtype):
  users, items, k = 17, 130, 5
  table, norms = cc.table_case(users, items, dtype)
  want = _topk(be, table[:, 3:70], norms[3:70], table[:, 60:130], norms[60:130], k, index_offset=60)
  assert _same(want, cc.restatement(table[:, 3:70], norms[3:70], table[:, 60:130], norms[60:130], k, index_offset=60))
  d_table, d_norms = _dev(be, table), _dev(be, norms)
  # two column ranges of one wider table
  got = be.item_topk(d_table[:, 3:70], d_norms[3:70], d_table[:, 60:130], d_norms[60:130], k, index_offset=60)
  assert _same((got[0].numpy(), got[1].numpy()), want)
  # sources from a table of another width (ldt != lds), strided norms, and operands whose inner stride is not 1
  wide = _dev(be, np.concatenate([table[:, 60:130], table[:, :9]], axis=1))
  got = be.item_topk(d_table[:, 3:70], d_norms[3:70], wide[:, :70], d_norms[60:130], k, index_offset=60)
  assert _same((got[0].numpy(), got[1].numpy()), want)
  transposed = _dev(be, np.ascontiguousarray(table.T))                     # [items, users]: its transpose has inner stride `users`
  every_other = _dev(be, np.repeat(norms, 2))
  got = be.item_topk(transposed.transpose()[:, 3:70], every_other[6:140:2], transposed.transpose()[:, 60:130], every_other[120:260:2], k,
                     index_offset=60)
  assert _same((got[0].numpy(), got[1].numpy()), want)
  got = be.item_topk(table[:, 3:70], norms[3:70].copy(), table[:, 60:130], norms[60:130].copy(), k, index_offset=60)   # host arrays
  assert _same((got[0].numpy(), got[1].numpy()), want)


@pytest.mark.parametrize('dtype', cc.DTYPES, **IDS)
def test_ties_and_special_values(be, dtype):
  dt = np.dtype(dtype)
  rng = np.random.default_rng(5)
  # two identical columns take the lower index first; an all-zero column: a row of +0 with indices 0 .. k - 1
  table = rng.standard_normal((33, 70)).astype(dt)
  table[:, 66] = table[:, 2]
  table[:, 40] = 0
  norms = cc.norms_of(table)
  sim, idx = _topk(be, table, norms, table, norms, 5)
  assert _same((sim, idx), cc.restatement(table, norms, table, norms, 5))
  for j in (2, 66):
    assert idx[j, :2].tolist() == [2, 66] and sim[j, 0] == sim[j, 1]
  assert idx[40].tolist() == [0, 1, 2, 3, 4] and sim[40].tobytes() == np.zeros(5, dt).tobytes()
  # many disjoint columns: long runs of exact-0 similarities, in ascending index
  disjoint = np.zeros((65, 130), dt)
  disjoint[np.arange(130) % 65, np.arange(130)] = rng.uniform(1, 2, 130).astype(dt) * np.where(np.arange(130) % 3 == 0, -1, 1)
  norms = cc.norms_of(disjoint)
  for k in (10, 128):
    sim, idx = _topk(be, disjoint, norms, disjoint, norms, k, splits=k % 3)
    assert _same((sim, idx), cc.restatement(disjoint, norms, disjoint, norms, k))
    j = 7                          # column 7 meets columns 7 and 72 only; every other similarity is +0 or -0
    zeros = idx[j][sim[j] == 0]
    assert len(zeros) >= k - 2 and zeros.tolist() == sorted(zeros.tolist()) and zeros[0] == 0
  # NaN and +-inf ratings, and norms of 0 and inf, follow np.nan_to_num
  special = rng.standard_normal((17, 66)).astype(dt)
  special[3, 5], special[4, 9], special[5, 11], special[:, 20] = np.nan, np.inf, -np.inf, 0
  norms = cc.norms_of(special)
  norms[30], norms[31] = 0, np.inf
  for k in (5, 66):
    sim, idx = _topk(be, special, norms, special, norms, k)
    assert _same((sim, idx), cc.restatement(special, norms, special, norms, k))
    assert not np.isnan(sim).any() and not np.isinf(sim).any()
  assert np.finfo(dt).max in sim and np.finfo(dt).min in sim
  # ns < k pads with -inf / -1; index_offset is added; no sources at all: all padding
  table, norms = cc.table_case(16, 65, dtype)
  sim, idx = _topk(be, table, norms, table[:, 60:63], norms[60:63], 5, index_offset=10 ** 10)
  assert _same((sim, idx), cc.restatement(table, norms, table[:, 60:63], norms[60:63], 5, index_offset=10 ** 10))
  assert (idx[:, 3:] == -1).all() and np.isneginf(sim[:, 3:]).all() and set(idx[0, :3]) == {10 ** 10, 10 ** 10 + 1, 10 ** 10 + 2}
  sim, idx = _topk(be, table, norms, table[:, :0], norms[:0], 3)
  assert (idx == -1).all() and np.isneginf(sim).all() and sim.shape == (65, 3)
  before = be.launches
  sim, idx = _topk(be, table[:, :0], norms[:0], table, norms, 3)                     # no targets: nothing is launched
  assert sim.shape == (0, 3) and idx.shape == (0, 3) and be.launches == before


@pytest.mark.parametrize('dtype', cc.DTYPES, **IDS)
def test_merge(be, dtype):
  dt = np.dtype(dtype)
  users, items, k = 33, 257, 10
  table, norms = cc.table_case(users, items, dtype)
  whole = _topk(be, table, norms, table, norms, k)
  # the candidates of source steps, merged, equal one call over all sources
  steps = [_topk(be, table, norms, table[:, lo:lo + 65], norms[lo:lo + 65], k, index_offset=lo) for lo in range(0, items, 65)]
  cand_sim, cand_idx = (np.concatenate([s[i] for s in steps], axis=1) for i in (0, 1))
  before = be.launches
  merged = be.item_topk_merge(_dev(be, cand_sim), _dev(be, cand_idx), k)
  assert be.launches - before == 1
  assert _same((merged[0].numpy(), merged[1].numpy()), whole)
  # shuffled candidates, padding in between, NaN candidates ignored
  rng = np.random.default_rng(11)
  order = rng.permutation(cand_sim.shape[1] + 7)
  padded_sim = np.concatenate([cand_sim, rng.standard_normal((items, 7)).astype(dt) + 5], axis=1)[:, order]
  padded_idx = np.concatenate([cand_idx, np.full((items, 7), -1, np.int64)], axis=1)[:, order]
  merged = be.item_topk_merge(_dev(be, padded_sim), _dev(be, padded_idx), k)
  assert _same((merged[0].numpy(), merged[1].numpy()), whole)
  assert _same((merged[0].numpy(), merged[1].numpy()), cc.restate_merge(padded_sim, padded_idx, k))
  with_nan = np.array(padded_sim)
  with_nan[:, 3] = np.nan
  merged = be.item_topk_merge(_dev(be, with_nan), _dev(be, padded_idx), k)
  assert _same((merged[0].numpy(), merged[1].numpy()), cc.restate_merge(with_nan, padded_idx, k))
  # cands < k, k = 128, one row, a strided view of wider candidate arrays
  for cands, kk in ((3, 10), (40, 128), (0, 4)):
    got = be.item_topk_merge(_dev(be, cand_sim[:, :cands]), _dev(be, cand_idx[:, :cands]), kk)
    assert _same((got[0].numpy(), got[1].numpy()), cc.restate_merge(cand_sim[:, :cands], cand_idx[:, :cands], kk)), cands
    assert (got[1].numpy()[:, cands:] == -1).all()
  d_sim, d_idx = _dev(be, cand_sim), _dev(be, cand_idx)
  got = be.item_topk_merge(d_sim[5:6, 2:30], d_idx[5:6, 2:30], k)
  assert _same((got[0].numpy(), got[1].numpy()), cc.restate_merge(cand_sim[5:6, 2:30], cand_idx[5:6, 2:30], k))
  got = be.item_topk_merge(d_sim[:0], d_idx[:0], k)
  assert got[0].shape == (0, k)


def test_refusals(be):
  f32 = np.zeros((7, 3), np.float32)
  n32 = np.ones(3, np.float32)
  with pytest.raises(TypeError, match='item_topk: dtype int32 .*astype first'):
    be.item_topk(f32.astype(np.int32), n32, f32, n32, 2)
  with pytest.raises(TypeError, match='item_topk: operands of two dtypes .*astype first'):
    be.item_topk(f32, n32, f32.astype(np.float64), n32, 2)
  with pytest.raises(ValueError, match='item_topk: targets and sources must be 2-D'):
    be.item_topk(f32[0], n32, f32, n32, 2)
  with pytest.raises(ValueError, match='item_topk: targets of 7 users against sources of 6'):
    be.item_topk(f32, n32, f32[:6], n32, 2)
  with pytest.raises(ValueError, match='item_topk: norms of shapes'):
    be.item_topk(f32, n32[:2], f32, n32, 2)
  for k in (0, 129):
    with pytest.raises(ValueError, match='item_topk: k = %d is outside 1 .. 128' % k):
      be.item_topk(f32, n32, f32, n32, k)
    with pytest.raises(ValueError, match='item_topk_merge: k = %d is outside 1 .. 128' % k):
      be.item_topk_merge(f32, np.zeros((7, 3), np.int64), k)
  with pytest.raises(ValueError, match='item_topk: splits = -1'):
    be.item_topk(f32, n32, f32, n32, 2, splits=-1)
  with pytest.raises(TypeError, match='float16 is not supported by item_topk_merge .*astype first'):
    be.item_topk_merge(f32.astype(np.float16), np.zeros((7, 3), np.int64), 2)
  with pytest.raises(TypeError, match='item_topk_merge: candidate indices of dtype int32'):
    be.item_topk_merge(f32, np.zeros((7, 3), np.int32), 2)
  with pytest.raises(ValueError, match='item_topk_merge: shapes'):
    be.item_topk_merge(f32, np.zeros((7, 4), np.int64), 2)
  # the launcher refuses through the same function, before any launch; the library itself refuses other dtypes
  out_s, out_i = devarray.empty((3, 2), np.float32), devarray.empty((3, 2), np.int64)
  d, dn = _dev(be, f32), _dev(be, n32)
  with pytest.raises(ValueError, match='item_topk: k = 200'):
    kernels.item_topk(d, dn, d, dn, 200, out_s, out_i)
  rc = _hip.extras().sp_item_topk(_hip.SP_I32, None, 3, None, 3, None, 3, None, 3, 7, 2, 0, 0, None, None, None, 0, None)
  assert rc != 0 and 'astype first' in _hip.lib().sp_last_error().decode()
  rc = _hip.extras().sp_item_topk_merge(_hip.SP_I64, None, None, 3, 3, 3, 2, None, None, None)
  assert rc != 0 and 'astype first' in _hip.lib().sp_last_error().decode()
