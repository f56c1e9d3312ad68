"""sp_nb_step (csrc/nb.hip) through HipBackend.nb_step and kernels.nb_step, against the oracle and the derived bound of
tests/nb_cases.py, and the naive Bayes driver on the device.

Shapes (tests/nb_cases.SHAPES), for the tiling that was built (include/spartan_hip_nb.h): a block is 64 rows, so m is 1
and on both sides of 64 and 128; the accumulation takes 4 rows at a time behind a ring of 8, 16 or 48 rows in flight (m = 1, 8, 9, 63, 65, 130); a lane of the row sums
takes the columns 64 apart and a panel is 64, 128 or 256 columns, chosen from label_size, d and the dtype (d = 1, 3, 63,
64, 65, 70, 130, 257, 300 with label_size = 1, 2, 5, 64, 128 give every width and up to five panels).  Under splits = 0
two ranges need 961 rows, so splits = 2 and 3 are forced at 130, 200 and 600 rows.  Nothing is larger than 600 x 300.
Measured shares of the bound are printed before each assertion (pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, devarray, kernels
from tests import nb_cases as nc
from tests import test_nb_example as ex

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
IDS = lambda s: '%dx%dx%d-%s' % s   # noqa: E731


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _framed(be, a, pad, fill=-77):
  """`a` as a row view of a wider device array (row stride a.shape[1] + pad): (view, the whole buffer, its host image)."""
  frame = np.full((a.shape[0] + 2, a.shape[1] + pad), fill, a.dtype)
  frame[1:a.shape[0] + 1, 1:a.shape[1] + 1] = a
  buf = be.from_numpy(frame)
  return buf[1:a.shape[0] + 1, 1:a.shape[1] + 1], buf, frame


def _step(be, x, labels, label_size, splits=0):
  s, df, bad = be.nb_step(be.from_numpy(np.ascontiguousarray(x)), be.from_numpy(np.ascontiguousarray(labels)), label_size,
                          splits=splits)
  return s.numpy(), df.numpy(), bad.numpy()


def _rows_z(be, x):
  """The kernel's own z of at most 128 rows: every row its own label."""
  m = x.shape[0]
  assert 1 <= m <= 128
  return _step(be, x, np.arange(m, dtype=np.int64), m, splits=1)[0]


def _kernel_z(be, x):
  return np.vstack([_rows_z(be, x[lo:lo + 128]) for lo in range(0, x.shape[0], 128)])


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', nc.SHAPES, ids=IDS)
def test_every_output_meets_the_derived_bound(be, shape, dtype):
  m, d, label_size, kind = shape
  dt = np.dtype(dtype)
  x, labels = nc.case(m, d, label_size, kind, dt)
  want = nc.oracle_of_case(m, d, label_size, kind, dt)
  before = be.launches
  s, df, bad = _step(be, x, labels, label_size)
  assert be.launches - before == 1          # (one per call: HipBackend.nb_step's docstring)
  nc.check_step(x, labels, label_size, s, df, bad, want=want, label='hip %s %s' % (shape, dt.name))
  # one range: the row-order sum of the kernel's own z, bit for bit
  z = _kernel_z(be, x)
  assert s.tobytes() == nc.row_order_sum(z, labels, label_size).tobytes()
  again = _step(be, x, labels, label_size)
  assert again[0].tobytes() == s.tobytes() and again[1].tobytes() == df.tobytes() and again[2].tobytes() == bad.tobytes()
  used = np.zeros(label_size, bool)
  used[labels] = True
  assert not np.any(s[~used])                 # a label nobody has: zeros


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', nc.SPLIT_SHAPES, ids=IDS)
def test_row_ranges_agree_within_the_bound(be, shape, dtype):
  m, d, label_size, kind = shape
  dt = np.dtype(dtype)
  x, labels = nc.case(m, d, label_size, kind, dt)
  want = nc.oracle_of_case(m, d, label_size, kind, dt)
  z = _kernel_z(be, x)
  nb = -(-m // 64)
  base = _step(be, x, labels, label_size, splits=1)
  assert base[0].tobytes() == nc.row_order_sum(z, labels, label_size).tobytes()
  assert base[0].tobytes() == _step(be, x, labels, label_size, splits=0)[0].tobytes()      # few rows: one range
  for splits in (2, 3, 64):
    s, df, bad = _step(be, x, labels, label_size, splits=splits)
    nc.check_step(x, labels, label_size, s, df, bad, want=want, label='hip %s %s splits=%d' % (shape, dt.name, splits))
    assert df.tobytes() == base[1].tobytes() and bad.tobytes() == base[2].tobytes()
    # the ranges' row-order sums, added in ascending range order onto range 0's
    ranges = min(splits, nb)
    cuts = [(g * nb // ranges) * 64 for g in range(ranges)] + [m]
    parts = [nc.row_order_sum(z[lo:hi], labels[lo:hi], label_size) for lo, hi in zip(cuts[:-1], cuts[1:])]
    acc = parts[0]
    for p in parts[1:]:
      acc = acc + p
    assert s.tobytes() == acc.tobytes(), splits
    assert _step(be, x, labels, label_size, splits=splits)[0].tobytes() == s.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_row_does_not_depend_on_its_neighbours(be, dtype):
  dt = np.dtype(dtype)
  x, _ = nc.case(130, 70, 5, 'random', dt, seed=1)
  z = _rows_z(be, x[:128])
  for lo, hi in ((0, 1), (5, 14), (60, 70), (64, 128)):
    assert _rows_z(be, x[lo:hi]).tobytes() == z[lo:hi].tobytes(), (lo, hi)
  other = np.array(x[:128])
  other[np.arange(128) != 77] *= 3                    # every neighbour changes, row 77 does not
  assert _rows_z(be, other)[77].tobytes() == z[77].tobytes()
  assert _rows_z(be, x[2:130])[:126].tobytes() == z[2:].tobytes()
  # z in the kernel is x / sqrt(q / d) with IEEE division and square root: within e_z of the exact value
  want = nc.oracle(x[:128], np.arange(128), 128)
  share = nc._ratio(np.abs(np.asarray(z, nc.LD) - want['z']), nc.eps_z(70, dt) * np.abs(np.asarray(want['z'], np.float64)))
  print('hip z %s: %.3g of e_z' % (dt.name, share))
  assert share <= 1.0


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_special_values(be, dtype):
  dt = np.dtype(dtype)
  x, labels = (np.array(a) for a in nc.case(130, 70, 5, 'random', dt))
  base = _step(be, x, labels, 5)
  zero = x.copy()
  zero[100] = 0
  for splits in (1, 3):
    s, df, bad = _step(be, zero, labels, 5, splits=splits)
    nan_rows = np.isnan(s).all(axis=1)
    assert nan_rows.tolist() == [l == labels[100] for l in range(5)] and not np.isnan(s[~nan_rows]).any()
    assert bad[0] == 0
    if splits == 1:
      assert s[~nan_rows].tobytes() == base[0][~nan_rows].tobytes()
    nc.check_step(zero, labels, 5, s, df, bad, label='hip zero row %s splits=%d' % (dt.name, splits))
  neg = x.copy()
  neg[3, 2], neg[9, 4], neg[70, 69] = -2.0, np.nan, -0.0
  s, df, bad = _step(be, neg, labels, 5)
  assert df[2] == (x[:, 2] > 0).sum() - (x[3, 2] > 0) and df[4] == (x[:, 4] > 0).sum() - (x[9, 4] > 0)
  assert np.isnan(s[labels[9]]).all()
  nc.check_step(neg, labels, 5, s, df, bad, label='hip negative and NaN entries %s' % dt.name)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_labels_out_of_range(be, dtype):
  dt = np.dtype(dtype)
  x, labels = nc.case(130, 70, 5, 'random', dt)
  base = _step(be, x, labels, 5)
  for wrong in (-1, 5, 2 ** 40, -2 ** 40):
    for rows in ((129,), (0, 64), (100, 12, 77)):
      lab = np.array(labels)
      lab[list(rows)] = wrong
      for splits in (1, 3):
        s, df, bad = _step(be, x, lab, 5, splits=splits)
        assert bad.tolist() == [min(rows) + 1] and df.tobytes() == base[1].tobytes()
        nc.check_step(x, lab, 5, s, df, bad, label='hip label %d at %s %s splits=%d' % (wrong, rows, dt.name, splits))
      keep = np.ones(130, bool)
      keep[list(rows)] = False
      assert _step(be, x, lab, 5, splits=1)[0].tobytes() == _step(be, x[keep], labels[keep], 5, splits=1)[0].tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_empty_shapes(be, dtype):
  dt = np.dtype(dtype)
  x, labels = nc.case(65, 7, 5, 'random', dt)
  before = be.launches
  s, df, bad = _step(be, x[:0], labels[:0], 5)
  assert be.launches == before                        # m = 0: nothing is launched
  assert s.shape == (5, 7) and s.dtype == dt and not s.any() and df.shape == (7,) and not df.any() and bad.tolist() == [0]
  s, df, bad = _step(be, x[:, :0], labels, 5)         # d = 0 is accepted
  assert s.shape == (5, 0) and df.shape == (0,) and bad.tolist() == [0]
  lab = np.array(labels)
  lab[40] = 9
  assert _step(be, x[:, :0], lab, 5)[2].tolist() == [41]      # ... and still reports a label out of range
  # the library takes m = 0 as well (the backend does not ask it to): zeros
  st, dft, badt = be.from_numpy(np.full((5, 7), 3, dt)), be.from_numpy(np.full(7, 3, np.int64)), be.from_numpy(np.full(1, 3, np.int64))
  kernels.nb_step(be.from_numpy(np.zeros((0, 7), dt)), be.from_numpy(np.zeros(0, np.int64)), 5, st, dft, badt)
  assert not st.numpy().any() and not dft.numpy().any() and not badt.numpy().any()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('pad', (3, 4))
def test_views_of_wider_buffers_give_the_same_bits(be, pad, dtype):
  dt = np.dtype(dtype)
  m, d, label_size = 130, 70, 5
  x, labels = nc.case(m, d, label_size, 'random', dt)
  for splits in (1, 3):
    s, df, bad = _step(be, x, labels, label_size, splits=splits)
    (xt, xbuf, xframe), (st, sbuf, sframe) = _framed(be, x, pad), _framed(be, np.zeros((label_size, d), dt), pad + 2)
    yt, ybuf, yframe = _framed(be, labels.reshape(m, 1), 2)
    assert tuple(yt.shape) == (m, 1) and yt.stride(0) == 3
    got = be.nb_step(xt, yt, label_size, splits=splits)         # the labels as an [m, 1] view of a wider array
    assert got[0].numpy().tobytes() == s.tobytes() and got[1].numpy().tobytes() == df.tobytes()
    assert got[2].numpy().tobytes() == bad.tobytes()
    dft, badt = be.empty((d,), np.int64), be.empty((1,), np.int64)
    kernels.nb_step(xt, be.from_numpy(labels.reshape(m, 1)), label_size, st, dft, badt, splits=splits)
    assert st.numpy().tobytes() == s.tobytes() and dft.numpy().tobytes() == df.tobytes() and badt.numpy().tobytes() == bad.tobytes()
    assert xbuf.numpy().tobytes() == xframe.tobytes() and ybuf.numpy().tobytes() == yframe.tobytes()    # inputs unchanged
    sframe[1:label_size + 1, 1:d + 1] = s
    assert sbuf.numpy().tobytes() == sframe.tobytes()                                                     # frame untouched


def test_refusals_launch_nothing(be):
  x, labels = nc.case(9, 3, 2, 'random', np.dtype(np.float32))
  xt, yt = be.from_numpy(x), be.from_numpy(labels)
  before = be.launches
  for bad in (x.astype(np.int32), x.astype(np.float16)):
    with pytest.raises(TypeError, match='astype'):
      be.nb_step(be.from_numpy(bad), yt, 2)
  for bad in (labels.astype(np.int32), labels.astype(np.float64)):
    with pytest.raises(TypeError, match='astype'):
      be.nb_step(xt, be.from_numpy(bad), 2)
  for size in (0, 129, -1):
    with pytest.raises(ValueError, match='label_size'):
      be.nb_step(xt, yt, size)
  with pytest.raises(ValueError, match=r'\(m, d\)'):
    be.nb_step(be.from_numpy(x.reshape(-1)), yt, 2)
  for bad in (labels[:8], labels.reshape(3, 3)):
    with pytest.raises(ValueError, match='labels of shape'):
      be.nb_step(xt, be.from_numpy(np.ascontiguousarray(bad)), 2)
  with pytest.raises(ValueError, match='splits'):
    be.nb_step(xt, yt, 2, splits=-1)
  s, df, bad = be.empty((2, 3), np.float32), be.empty((3,), np.int64), be.empty((1,), np.int64)
  with pytest.raises(TypeError, match='astype'):
    kernels.nb_step(xt, yt, 2, be.empty((2, 3), np.float64), df, bad)
  with pytest.raises(ValueError, match='targets of shapes'):
    kernels.nb_step(xt, yt, 2, be.empty((3, 3), np.float32), df, bad)
  with pytest.raises(ValueError, match='targets of shapes'):
    kernels.nb_step(xt, yt, 2, s, be.empty((4,), np.int64), bad)
  with pytest.raises(TypeError, match='int64'):
    kernels.nb_step(xt, yt, 2, s, be.empty((3,), np.int32), bad)
  assert be.launches == before
  # the library's own refusals
  lib, err = _hip.extras(), _hip.lib().sp_last_error
  f32 = _hip.SP_F32

  def step(dtype=f32, ldx=3, m=9, d=3, label_size=2, splits=0, lds=3, ws_bytes=0):
    return lib.sp_nb_step(dtype, None, ldx, m, d, None, label_size, splits, None, lds, None, None, None, ws_bytes, None)

  for dtype in (_hip.SP_I32, _hip.SP_F16, _hip.SP_I64):
    assert step(dtype=dtype) != 0 and 'astype' in err().decode()
  for size in (0, 129, -5):
    assert step(label_size=size) != 0 and 'label_size' in err().decode()
  assert step(ldx=2) != 0 and 'bad shape' in err().decode()
  assert step(lds=2) != 0 and 'bad shape' in err().decode()
  for kw in (dict(m=-1), dict(d=-1, ldx=0, lds=0), dict(splits=-1)):
    assert step(**kw) != 0 and 'bad shape' in err().decode()
  assert step() != 0 and 'required' in err().decode()         # (no operands: refused before anything is launched)
  rc = lib.sp_nb_step(f32, None, 3, 9, 3, None, 2, 0, s.data_ptr(), 3, df.data_ptr(), bad.data_ptr(), None, 0, None)
  assert rc != 0 and 'required' in err().decode()              # targets, but neither X nor labels
  # a workspace that is missing or too small
  need = lib.sp_nb_step_workspace_bytes(f32, 9, 3, 2, 0)
  assert need == 256
  ws = be.empty((need,), np.uint8)
  marks = np.full((2, 3), -5, np.float32)
  s = be.from_numpy(marks)
  for ptr, size in ((ws.data_ptr(), need - 1), (None, 0), (None, need)):
    rc = lib.sp_nb_step(f32, xt.data_ptr(), 3, 9, 3, yt.data_ptr(), 2, 0, s.data_ptr(), 3, df.data_ptr(), bad.data_ptr(), ptr,
                        size, None)
    assert rc != 0 and 'workspace' in err().decode()
  assert s.numpy().tobytes() == marks.tobytes()               # nothing was written
  rc = lib.sp_nb_step(f32, xt.data_ptr(), 3, 9, 3, yt.data_ptr(), 2, 0, s.data_ptr(), 3, df.data_ptr(), bad.data_ptr(),
                      ws.data_ptr(), need, devarray.current_stream().ptr)
  assert rc == 0 and s.numpy().tobytes() == _step(be, x, labels, 2)[0].tobytes()


# ---- the driver on the device -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('workers', (1, 4))
def test_the_driver_reproduces_the_reference_gpu(workers, dtype):
  ex.check_driver('hip', workers, dtype)


def test_the_driver_takes_flat_labels_gpu():
  ex.check_driver('hip', 4, np.float64, labels_2d=False)


def test_df_is_exact_and_integer_data_takes_the_float64_path_gpu():
  ex.check_df_and_integers('hip')


def test_driver_refusals_gpu():
  ex.check_refusals('hip')
