"""tests/cf_cases.py checked on the CPU: the oracle against a plain double loop, the NumPy body of the tile functions
(examples/cf/_cf.py) against the derived bound and, byte for byte, against the ordered restatement, that the bound is
not vacuous, that the generated cases leave few rows to the "values only" comparison, the bindings of the library's
header, its workspace sizes and the shared refusals.  Measured shares of the bounds are printed before each assertion
(pytest -s)."""
import ctypes
import os
import re

import numpy as np
import pytest

from spartan_amd import _hip, tile_checks
from spartan_amd.examples.cf import _cf
from tests import cf_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = dict(ids=lambda d: np.dtype(d).name)


def test_the_oracle_agrees_with_a_plain_double_loop():
  table, norms = cc.table_case(7, 5, np.float64)
  sim, bound = cc.oracle(table, norms, table, norms)
  for j in range(5):
    for i in range(5):
      dot = sum(cc.LD(table[u, j]) * cc.LD(table[u, i]) for u in range(7))
      mag = sum(abs(cc.LD(table[u, j]) * cc.LD(table[u, i])) for u in range(7))
      den = cc.LD(norms[j]) * cc.LD(norms[i])
      assert abs(sim[j, i] - dot / den) <= 8 * np.finfo(cc.LD).eps * mag / den
      assert abs(bound[j, i] - cc.gamma(9, np.float64) * mag / den) <= 1e-3 * bound[j, i]
  assert abs(sim[2, 2] - 1) < 1e-15                       # an item against itself, with its own rounded norm


@pytest.mark.parametrize('dtype', cc.DTYPES, **IDS)
def test_the_numpy_body_meets_the_bound_and_equals_the_restatement(dtype):
  worst, unclear, rows = 0.0, 0, 0
  for users in cc.USERS:
    for items in cc.ITEMS:
      table, norms = cc.table_case(users, items, dtype)
      exact, bound = cc.case_oracle(users, items, dtype)
      stated = cc.case_similarities(users, items, dtype)
      for k in cc.KS:
        label = 'item_topk_numpy users=%d items=%d k=%d %s' % (users, items, k, np.dtype(dtype).name)
        sim, idx = _cf.item_topk_numpy(table, norms, table, norms, k)
        assert sim.dtype == np.dtype(dtype) and idx.dtype == np.int64
        w, v, m = cc.check_topk(sim, idx, exact, bound, k, label=label)
        worst = max(worst, w)
        if users >= 2:
          unclear, rows = unclear + v, rows + m
        want = cc.restated_selection(stated, k)
        assert sim.tobytes() == want[0].tobytes() and idx.tobytes() == want[1].tobytes(), label
  print('item_topk_numpy %s: at %.3g of the bound; %d of %d rows by values only' % (np.dtype(dtype).name, worst, unclear, rows))
  assert worst <= 1.0
  assert unclear <= cc.VALUES_ONLY_SHARE * rows, (unclear, rows)


@pytest.mark.parametrize('dtype', cc.DTYPES, **IDS)
def test_bands_offsets_and_merged_steps_equal_the_whole(dtype):
  table, norms = cc.table_case(33, 130, dtype)
  k = 10
  whole = _cf.item_topk_numpy(table, norms, table, norms, k)
  for lo in (1, 63, 64, 65):
    band = _cf.item_topk_numpy(table[:, lo:lo + 40], norms[lo:lo + 40], table, norms, k)
    assert band[0].tobytes() == whole[0][lo:lo + 40].tobytes() and band[1].tobytes() == whole[1][lo:lo + 40].tobytes()
  cand = [_cf.item_topk_numpy(table, norms, table[:, lo:lo + 33], norms[lo:lo + 33], k, index_offset=lo)
          for lo in range(0, 130, 33)]
  cand_sim, cand_idx = (np.concatenate([c[i] for c in cand], axis=1) for i in (0, 1))
  for merged in (_cf._select(cand_sim, cand_idx, cand_idx >= 0, k), cc.restate_merge(cand_sim, cand_idx, k)):
    assert merged[0].tobytes() == whole[0].tobytes() and merged[1].tobytes() == whole[1].tobytes()
  few = _cf.item_topk_numpy(table, norms, table[:, 5:8], norms[5:8], k, index_offset=5)     # ns < k: padding
  assert (few[1][:, 3:] == -1).all() and np.isneginf(few[0][:, 3:]).all() and set(few[1][0, :3]) == {5, 6, 7}


@pytest.mark.parametrize('dtype', cc.DTYPES, **IDS)
def test_the_bound_is_not_vacuous(dtype):
  """One user's product dropped from a pair moves the similarity by more than the bound."""
  table, norms = cc.table_case(33, 65, dtype)
  exact, bound = cc.oracle(table, norms, table, norms)
  short = np.array(table)
  short[17] = 0
  got = _cf.similarities_numpy(short, norms, short, norms)
  moved = np.abs(np.asarray(got, cc.LD) - exact) > bound
  assert moved.mean() > 0.99


def test_special_values_follow_nan_to_num():
  for dtype in cc.DTYPES:
    dt = np.dtype(dtype)
    t = np.array([[1, 0, np.inf, 2, 1], [2, 0, 1, np.nan, 2]], dt)
    n = np.array([1, 0, 1, 1, 0], dt)
    sim = _cf.similarities_numpy(t, n, t, n)
    assert sim[1].tobytes() == np.zeros(5, dt).tobytes()                   # an item of norm 0: +0 with everything
    assert sim[0, 2] == np.finfo(dt).max and sim[0, 3] == 0 and not np.signbit(sim[0, 3])      # +inf and NaN
    neg = _cf.similarities_numpy(-t[:, :1], n[:1], t, n)
    assert neg[0, 2] == np.finfo(dt).min
    top, idx = _cf.item_topk_numpy(t, n, t, n, 3)
    assert idx[1].tolist() == [0, 1, 2] and top[1].tobytes() == np.zeros(3, dt).tobytes()


def test_the_header_declares_what_is_bound():
  text = open(os.path.join(ROOT, 'include', 'spartan_hip_cf.h')).read()
  code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  names = sorted(set(re.findall(r'\b(sp_[a-z0-9_]+)\s*\(', code)))
  assert names == sorted(_hip.EXPORTS_CF) == ['sp_item_topk', 'sp_item_topk_merge', 'sp_item_topk_workspace_bytes']
  assert int(re.search(r'#define SP_CF_MAX_K (\d+)\b', text).group(1)) == _hip.CF_MAX_K == cc.MAX_K
  others = set(_hip.EXPORTS)
  for header, symbols in _hip._EXTRAS_ABI.items():
    if header != 'spartan_hip_cf.h':
      others |= set(symbols)
  assert not set(names) & others
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]


def test_workspace_sizes():
  size = _hip.extras().sp_item_topk_workspace_bytes      # host code: sizes need no device
  f32, f64 = _hip.SP_F32, _hip.SP_F64
  for code, es in ((f32, 4), (f64, 8)):
    assert size(code, 200, 257, 257, 10, 1) == 0          # nothing is split: no workspace
    assert size(code, 200, 64, 64, 5, 0) == 0             # one block of sources: the library does not cut it
    assert size(code, 200, 0, 257, 10, 3) == 0            # no targets
    assert size(code, 200, 257, 0, 10, 3) == 0            # no sources: one (empty) range
    for s in (2, 3, 64):
      r = min(s, 257)
      assert size(code, 200, 257, 257, 10, s) == -(-257 * r * 10 * es // 256) * 256 + 257 * r * 10 * 8
    sizes = [size(code, 200, 257, 257, 10, s) for s in range(1, 300)]
    assert sizes == sorted(sizes) and sizes[256] == sizes[-1]            # monotone in splits; at most ns ranges
  # the library's own choice (the header states it), and cf_cases' copy of it
  for m, ns, k in ((800, 800, 10), (8192, 8192, 10), (64, 100000, 128), (257, 257, 10), (257, 257, 64), (130, 130, 1), (1, 300, 5), (65, 65, 5), (64, 64, 1), (16384, 16384, 10), (100, 5000, 128)):
    assert size(f32, 9, m, ns, k, 0) == size(f32, 9, m, ns, k, cc.ranges_of(m, ns, k, 0)), (m, ns, k)
  assert [cc.ranges_of(m, ns, k, 0) for m, ns, k in ((800, 800, 10), (257, 257, 10), (257, 257, 64), (130, 130, 1))] == [13, 5, 2, 3]
  assert [cc.ranges_of(257, 257, 10, s) for s in (1, 2, 3, 64, 300)] == [1, 2, 3, 64, 257]
  assert size(f32, 8000, 800, 800, 10, 0) == size(f32, 8000, 800, 800, 10, 13)
  assert size(f32, 9, 8192, 8192, 10, 0) == size(f32, 9, 8192, 8192, 10, 4)
  assert size(f32, 9, 64, 100000, 128, 0) == size(f32, 9, 64, 100000, 128, 63)
  assert size(_hip.SP_I32, 9, 9, 9, 5, 2) == 0 == size(f32, 9, 9, 9, 0, 2) == size(f32, 9, 9, 9, 129, 2) == size(f32, 9, 9, 9, 5, -1)


def test_operand_refusals():
  f32, f64 = np.dtype(np.float32), np.dtype(np.float64)
  check = tile_checks.check_item_topk_operands
  assert check([f64] * 4, (7, 3), (3,), (7, 9), (9,), 5) == (f64, 7, 3, 9, 5, 0)
  assert check([f32] * 4, (0, 3), (3,), (0, 0), (0,), 128, 4) == (f32, 0, 3, 0, 128, 4)
  for bad in (np.int32, np.float16, np.complex128, object):
    with pytest.raises(TypeError, match='astype first'):
      check([f64, f64, np.dtype(bad), f64], (7, 3), (3,), (7, 9), (9,), 5)
  with pytest.raises(TypeError, match='two dtypes.*astype first'):
    check([f64, f64, f32, f32], (7, 3), (3,), (7, 9), (9,), 5)
  for t, s in (((7,), (7, 9)), ((7, 3), (7, 9, 1)), ((7, 3, 1), (7, 9))):
    with pytest.raises(ValueError, match='2-D'):
      check([f64] * 4, t, (3,), s, (9,), 5)
  with pytest.raises(ValueError, match='users'):
    check([f64] * 4, (7, 3), (3,), (8, 9), (9,), 5)
  for tn, sn in (((4,), (9,)), ((3,), (9, 1)), ((3, 1), (9,)), ((3,), (8,))):
    with pytest.raises(ValueError, match='norms'):
      check([f64] * 4, (7, 3), tn, (7, 9), sn, 5)
  for k in (0, -1, 129):
    with pytest.raises(ValueError, match='k = .* outside 1 .. 128'):
      check([f64] * 4, (7, 3), (3,), (7, 9), (9,), k)
  with pytest.raises(ValueError, match='splits'):
    check([f64] * 4, (7, 3), (3,), (7, 9), (9,), 5, splits=-1)
  # the NumPy body refuses through the same function
  with pytest.raises(ValueError, match='k = '):
    _cf.check_operands([f64] * 4, (7, 3), (3,), (7, 9), (9,), 200)
