"""sp_canopy and sp_pdf_label (csrc/canopy.hip) through HipBackend.canopy / pdf_label and the launchers against the
NumPy bodies of examples/_canopy.py, byte for byte, in both dtypes: the kernels do the same operations in the same order
(include/spartan_hip_canopy.h), so every comparison -- also one that is a last bit away from a threshold -- falls alike.

Shapes, for the kernel that was built: n = 0, 1, 63, 64, 65 and 130 rows sit on both sides of a block of 64 rows;
200 separated rows make 200 canopies, past one and two tiles of 64 canopies; d = 1, 2, 16, 17 and 35 sit on both sides
of the distance tile's chunks of 16 features; chains = 1, 3 and n leave chains of one row; k = 0, 1, 64, 65 and 130
centres sit on both sides of a sweep of 64.  Nothing is larger."""
import ctypes

import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, kernels
from spartan_amd.examples import _canopy
from tests import canopy_cases as case

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
dtype_ids = dict(ids=lambda d: np.dtype(d).name)
NS = (0, 1, 63, 64, 65, 130)
DS = (1, 2, 16, 17, 35)
THRESHOLDS = ((0.05, 0.03), (0.03, 0.05), (0.04, 0.04))      # (t1, t2) per feature: t1 > t2, t1 < t2, t1 = t2


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _points(n, d, dtype, seed=0):
  """n rows around 5 blobs in the unit cube, spread 0.1: squared distances near 0.02 d inside a blob."""
  rng = np.random.RandomState(100 + seed)
  blobs = rng.rand(5, d)
  return np.ascontiguousarray((blobs[rng.randint(0, 5, n)] + 0.1 * rng.randn(n, d)).astype(dtype))


def _check(be, x, t1, t2, chains, cap=None, launches=1):
  before = be.launches
  got = be.canopy(be.from_numpy(x), t1, t2, chains=chains, cap=cap)
  assert be.launches - before == launches
  want = _canopy.canopy_numpy(x, t1, t2, chains)
  for g, w, name in zip(got, want, ('centers', 'counts', 'rows')):
    assert case.same(g, w), (name, x.shape, chains, t1, t2)
  return got


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('n', NS)
def test_rows_and_chains(be, n, dtype):
  for d in (2, 17):
    x = _points(n, d, dtype)
    for chains in sorted(set((1, 3, max(n, 1)))):
      for t1, t2 in THRESHOLDS:
        got = _check(be, x, t1 * d, t2 * d, chains)
        if n >= 63 and chains == 1:
          assert 1 < len(got[0]) < n and got[1].max() > 1       # canopies that observe, rows that are bound


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('d', DS)
def test_features(be, d, dtype):
  x = _points(130, d, dtype, seed=d)
  for chains in (1, 3):
    got = _check(be, x, 0.05 * d, 0.03 * d, chains)
  again = be.canopy(be.from_numpy(x), 0.05 * d, 0.03 * d, chains=3)           # a repeated call: the same bytes
  assert all(case.same(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_more_canopies_than_two_tiles(be, dtype):
  """200 rows one apart on a line, shuffled: t2 = 0.5 binds nobody, t1 = 4.5 observes the later rows at distance 1 and
  2.  The canopies pass 64 and 128 inside the run; with t1 = 0.5 as well every canopy stays alone."""
  order = np.random.RandomState(5).permutation(200)
  x = np.zeros((200, 3), dtype)
  x[:, 1] = order
  got = _check(be, x, 4.5, 0.5, 1)
  assert got[2].tolist() == list(range(200)) and 1 < got[1].max() <= 5
  got = _check(be, x, 0.5, 0.5, 1)
  assert got[1].tolist() == [1] * 200 and case.same(got[0], x)
  _check(be, x, 4.5, 0.5, 3)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_exact_thresholds_duplicates_and_nan(be, dtype):
  """Integer coordinates: a squared distance exactly equal to the threshold neither binds nor is observed (strict <);
  a duplicate of a creating row is observed; a row with a NaN is a canopy of its own."""
  x = np.array([[0, 0], [2, 0], [0, 0], [1, 0], [3, 0], [np.nan, 0], [0, 1]], dtype)
  centers, counts, rows = _check(be, x, 4, 4, 1)
  assert rows.tolist() == [0, 1, 5] and counts.tolist() == [4, 3, 1]
  assert case.same(centers, np.array([[1 / 4, 1 / 4], [2, 0], [np.nan, 0]], dtype))
  assert _check(be, x[:5], 1, 5, 1)[2].tolist() == [0, 4]
  assert _check(be, x[:5], 5, 1, 1)[1].tolist() == [4, 4, 2, 1]
  # 70 copies of three rows, across a block boundary: three canopies observe everything
  rep = np.ascontiguousarray(np.tile(np.array([[0, 0], [3, 0], [0, 3]], dtype), (70, 1)))
  centers, counts, rows = _check(be, rep, 1, 1, 1)
  assert rows.tolist() == [0, 1, 2] and counts.tolist() == [70, 70, 70]
  # NaN rows inside blob data, in both halves of a block pair
  x = _points(130, 3, dtype)
  x[7, 1] = x[100, 0] = np.nan
  got = _check(be, x, 0.15, 0.09, 1)
  assert {7, 100} <= set(got[2].tolist())


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_strided_and_transposed_views(be, dtype):
  n, d = 130, 5
  x = _points(n, d, dtype)
  want = _canopy.canopy_numpy(x, 0.25, 0.15, 3)
  centres = np.ascontiguousarray(want[0][:7])
  want_labels = _canopy.pdf_label_numpy(x, centres)
  # ldx = d + 3: a row view of a wider array, taken as it is
  wide = np.full((n, d + 3), 7.0, dtype)
  wide[:, :d] = x
  wide_t = be.from_numpy(wide)
  view = wide_t[:, :d]
  assert view.stride(0) == d + 3 and be._unit_rows(view) is view
  before = be.launches
  got = be.canopy(view, 0.25, 0.15, chains=3)
  assert be.launches - before == 1 and all(case.same(a, b) for a, b in zip(got, want))
  wide_c = be.from_numpy(np.concatenate([centres, np.full((7, 2), 9.0, dtype)], axis=1))
  before = be.launches
  labels = be.pdf_label(view, wide_c[:, :d])
  assert be.launches - before == 1 and case.same(labels.numpy(), want_labels)
  assert wide_t.numpy().tobytes() == wide.tobytes()                        # no operand is written
  # transposed: copied first, the same bytes, still one launch each
  xt = be.from_numpy(np.ascontiguousarray(x.T))
  ct = be.from_numpy(np.ascontiguousarray(centres.T))
  before = be.launches
  got = be.canopy(xt.t(), 0.25, 0.15, chains=3)
  labels = be.pdf_label(xt.t(), ct.t())
  assert be.launches - before == 2
  assert all(case.same(a, b) for a, b in zip(got, want)) and case.same(labels.numpy(), want_labels)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_cap_overflow_is_reported_and_retried_once(be, dtype):
  n, d, chains = 130, 3, 3
  x = _points(n, d, dtype)
  want = _canopy.canopy_numpy(x, 0.15, 0.09, chains)
  per_chain = [int(((want[2] >= lo) & (want[2] < hi)).sum()) for lo, hi in case.chain_rows(n, chains)]
  assert min(per_chain) > 2
  # at the C-ABI: cap = 2 does not suffice for any chain, cap = the most any chain needs does
  xt = be.from_numpy(x)
  for cap in (2, max(per_chain)):
    slots = chains * cap
    centers, counts = be.empty((slots, d), dtype), be.empty((slots,), np.int64)
    rows, num = be.empty((slots,), np.int64), be.empty((chains,), np.int64)
    kernels.canopy(xt, 0.15, 0.09, chains, cap, centers, counts, rows, num)
    assert num.numpy().tolist() == ([-1] * chains if cap == 2 else per_chain)
  keep = np.concatenate([np.arange(c * cap, c * cap + m) for c, m in enumerate(per_chain)])
  assert case.same(centers.numpy()[keep], want[0]) and case.same(counts.numpy()[keep], want[1])
  assert case.same(rows.numpy()[keep], want[2])
  # the backend's one retry gives the uncapped bytes
  _check(be, x, 0.15, 0.09, chains, cap=2, launches=2)
  _check(be, x, 0.15, 0.09, chains, cap=max(per_chain), launches=1)


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
@pytest.mark.parametrize('k', (0, 1, 64, 65, 130))
def test_pdf_label(be, k, dtype):
  for n, d in ((0, 3), (1, 3), (65, 2), (130, 17), (64, 35)):
    x = _points(n, d, dtype, seed=1)
    centres = _points(k, d, dtype, seed=2)
    if k > 3:
      centres[k // 2] = centres[1]                       # equal centres: the lower index wins
      centres[3, 0] = np.nan                             # a centre whose every pdf is NaN
    before = be.launches
    labels = be.pdf_label(be.from_numpy(x), be.from_numpy(centres))
    assert be.launches - before == (1 if n else 0)
    got = labels.numpy()
    assert case.same(got, _canopy.pdf_label_numpy(x, centres)), (n, d, k)
    if k == 0:
      assert got.tolist() == [-1] * n
    elif k > 3:
      assert not set(got.tolist()) & {3, k // 2}


@pytest.mark.parametrize('dtype', DTYPES, **dtype_ids)
def test_pdf_label_ties_and_nan_rows(be, dtype):
  """1 + 1e-20 rounds to 1: the farther centre, listed first, ties with the nearer one and wins -- an arg-min of the
  distance would say 1.  A row with a NaN has no pdf that wins: -1."""
  x = np.array([[0.0, 0.0], [5.0, 5.0], [np.nan, 1.0], [0.0, 0.0]], dtype)
  centres = np.array([[1e-10, 0.0], [0.0, 0.0], [5.0, 5.0]], dtype)
  got = be.pdf_label(be.from_numpy(x), be.from_numpy(centres)).numpy()
  assert got.tolist() == [0, 2, -1, 0] and case.same(got, _canopy.pdf_label_numpy(x, centres))
  # the tie across the 16 threads of a row and across two sweeps: 130 equal centres, then the nearer one at the end
  many = np.zeros((131, 2), dtype)
  many[:130, 0] = 1e-10
  got = be.pdf_label(be.from_numpy(x), be.from_numpy(many)).numpy()
  assert got.tolist() == [0, 0, -1, 0] and case.same(got, _canopy.pdf_label_numpy(x, many))


def test_the_c_abi_refuses_and_launches_nothing(be):
  """Every pointer is a real buffer of the right size, so only the scalar under test is wrong."""
  lib = _hip.extras()
  n, d, chains, cap = 9, 3, 2, 5
  x = _points(n, d, np.float32)
  xt = be.from_numpy(x)
  centers, counts = be.empty((chains * cap, d), np.float32), be.empty((chains * cap,), np.int64)
  rows, num = be.empty((chains * cap,), np.int64), be.from_numpy(np.full(chains, 77, np.int64))
  ws = be.empty((4096,), np.uint8)
  labels = be.from_numpy(np.full(n, 77, np.int32))
  p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
  f32 = _hip.SP_F32
  good = dict(dtype=f32, X=p(xt), ldx=d, n=n, d=d, t1=0.3, t2=0.2, chains=chains, cap=cap, centers=p(centers), ldc=d,
              counts=p(counts), rows=p(rows), num=p(num), ws=p(ws), ws_bytes=4096)

  def canopy(**kw):
    a = dict(good, **kw)
    return lib.sp_canopy(a['dtype'], a['X'], a['ldx'], a['n'], a['d'], a['t1'], a['t2'], a['chains'], a['cap'], a['centers'],
                         a['ldc'], a['counts'], a['rows'], a['num'], a['ws'], a['ws_bytes'], None)

  bad = [dict(dtype=_hip.SP_I32), dict(dtype=_hip.SP_F16), dict(ldx=d - 1), dict(ldc=d - 1), dict(d=0, ldx=0), dict(n=-1),
         dict(chains=0), dict(chains=-3), dict(cap=0), dict(t1=float('inf')), dict(t1=float('nan')), dict(t2=float('nan')),
         dict(t2=1e60), dict(X=None), dict(centers=None), dict(counts=None), dict(rows=None), dict(num=None), dict(ws=None),
         dict(ws_bytes=lib.sp_canopy_workspace_bytes(f32, n, d, chains, cap) - 1)]
  for kw in bad:
    assert canopy(**kw) != 0, kw
    assert 'sp_canopy' in _hip.lib().sp_last_error().decode()
  be.synchronize()
  assert num.numpy().tolist() == [77] * chains                      # nothing was launched
  assert canopy(dtype=_hip.SP_F64, t2=1e60, n=0, X=None) == 0      # finite in float64; n = 0 is accepted
  be.synchronize()
  assert num.numpy().tolist() == [0] * chains                       # ... and every chain reports no canopy

  cen = be.from_numpy(x[:2].copy())
  goodl = dict(dtype=f32, X=p(xt), ldx=d, n=n, C=p(cen), ldc=d, k=2, d=d, labels=p(labels))

  def label(**kw):
    a = dict(goodl, **kw)
    return lib.sp_pdf_label(a['dtype'], a['X'], a['ldx'], a['n'], a['C'], a['ldc'], a['k'], a['d'], a['labels'], None)

  for kw in (dict(dtype=_hip.SP_I64), dict(n=-1), dict(k=-1), dict(k=2 ** 31), dict(d=0), dict(ldx=d - 1), dict(ldc=d - 1),
             dict(X=None), dict(C=None), dict(labels=None)):
    assert label(**kw) != 0, kw
    assert 'sp_pdf_label' in _hip.lib().sp_last_error().decode()
  be.synchronize()
  assert labels.numpy().tolist() == [77] * n
  assert label(n=0, X=None, labels=None) == 0                       # nothing to do
  assert label(k=0, C=None) == 0
  be.synchronize()
  assert labels.numpy().tolist() == [-1] * n
