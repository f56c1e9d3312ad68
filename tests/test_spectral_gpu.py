"""sp_affinity_degree / sp_affinity_matrix (csrc/spectral.hip) through HipBackend and kernels, against the oracle and the
derived bound of tests/spectral_cases.py, and the spectral-clustering driver on the device.

Shapes (tests/spectral_cases.SHAPES), for the tiling that was built (include/spartan_hip_spectral.h): tiles of 64 x 64, so
m and n are 1 and on both sides of 64 and 128; four columns to a thread (n = 5, 63, 65, 129, 130); the features come in
chunks of 16 (d = 0, 1, 2, 3, 15, 16, 17, 33); bands that start inside the points (r0 = 3, 64, 127, 200, 383); n = 449 is
the smallest whose columns are cut into two ranges, added by the combine kernel.  Nothing is larger than 300 x 600.
Measured shares of the bound are printed before each assertion (pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, kernels
from tests import spectral_cases as sc
from tests import test_spectral_example as ex

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _framed(be, a, pad, fill=-77.0):
  """`a` as a row view of a wider device array (row stride a.shape[1] + pad): (view, the whole buffer, its host image)."""
  frame = np.full((a.shape[0] + 2, a.shape[1] + pad), fill, a.dtype)
  frame[1:a.shape[0] + 1, 1:a.shape[1] + 1] = a
  buf = be.from_numpy(frame)
  return buf[1:a.shape[0] + 1, 1:a.shape[1] + 1], buf, frame


def _pipeline(be, y, r0, m, metric, gamma=1.0):
  """(D of the band, D of all points, A of the band, L of the band) as host arrays, chained as the driver chains them."""
  yt = be.from_numpy(np.ascontiguousarray(y))
  xt = be.from_numpy(np.ascontiguousarray(y[r0:r0 + m]))
  deg_all = be.affinity_degree(yt, yt, metric, gamma).numpy()
  deg = be.affinity_degree(xt, yt, metric, gamma).numpy()
  a = be.affinity_matrix(xt, r0, yt, metric, gamma).numpy()
  lap = be.affinity_matrix(xt, r0, yt, metric, gamma, scale=be.from_numpy(sc.scale_of(deg_all))).numpy()
  return deg, deg_all, a, lap


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('metric', sc.METRICS)
@pytest.mark.parametrize('shape', sc.SHAPES, ids=lambda s: '%dx%dx%d+%d' % s)
def test_every_output_meets_the_derived_bound(be, shape, metric, dtype):
  m, n, d, r0 = shape
  y = sc.case(n, d, np.dtype(dtype))
  want = sc.oracle_of_case(n, d, np.dtype(dtype), metric)
  before = be.launches
  deg, deg_all, a, lap = _pipeline(be, y, r0, m, metric)
  assert be.launches - before == 4          # (one per call: the docstrings of HipBackend.affinity_degree / _matrix)
  assert deg.tobytes() == deg_all[r0:r0 + m].tobytes()          # a band's degrees are the whole's, bit for bit
  sc.check(y, r0, m, metric, want, deg=deg, a=a, lap=lap, label='hip %s %s %s' % (shape, metric, np.dtype(dtype).name))
  sc.check(y, 0, n, metric, want, deg=deg_all, label='hip %s %s %s, all rows' % (shape, metric, np.dtype(dtype).name))
  if n >= 2 and r0 == 0 and d > 0:
    assert a[0, 1] == (1 if metric == 'rbf' else 0)               # points 0 and 1 are the same point
  if m == n:
    assert a.tobytes() == a.T.tobytes() and lap.tobytes() == lap.T.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('metric', sc.METRICS)
def test_a_band_computed_alone_gives_the_bits_of_the_whole(be, metric, dtype):
  n, d = 130, 5
  y = sc.case(n, d, np.dtype(dtype), seed=1)
  deg, _, a, lap = _pipeline(be, y, 0, n, metric)
  assert a.tobytes() == a.T.tobytes() and lap.tobytes() == lap.T.tobytes()
  for lo, hi in ((0, 15), (15, 64), (64, 65), (65, 130)):
    deg_b, _, a_b, lap_b = _pipeline(be, y, lo, hi - lo, metric)
    assert deg_b.tobytes() == deg[lo:hi].tobytes(), (lo, hi)
    assert a_b.tobytes() == a[lo:hi].tobytes() and lap_b.tobytes() == lap[lo:hi].tobytes(), (lo, hi)
  again = _pipeline(be, y, 0, n, metric)
  assert again[0].tobytes() == deg.tobytes() and again[2].tobytes() == a.tobytes() and again[3].tobytes() == lap.tobytes()
  # with two column ranges as well: n = 449
  y = sc.case(449, 3, np.dtype(dtype))
  yt = be.from_numpy(y)
  whole = be.affinity_degree(yt, yt, metric, 1.0).numpy()
  for lo, hi in ((0, 1), (60, 130), (383, 449)):
    assert be.affinity_degree(be.from_numpy(np.ascontiguousarray(y[lo:hi])), yt, metric, 1.0).numpy().tobytes() \
        == whole[lo:hi].tobytes(), (lo, hi)
  assert be.affinity_degree(yt, yt, metric, 1.0).numpy().tobytes() == whole.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_identical_points_a_far_point_and_a_single_point(be, dtype):
  dt = np.dtype(dtype)
  y = np.array(sc.case(70, 3, dt, seed=2))
  y[40] = y[7]                                            # two identical points, 33 apart
  for metric in sc.METRICS:
    deg, _, a, lap = _pipeline(be, y, 0, 70, metric)
    same = 1 if metric == 'rbf' else 0
    assert a[40, 7] == same and a[7, 40] == same
    assert a[40].tobytes() == a[7].tobytes() and deg[40] == deg[7]
    assert np.delete(lap[40], (7, 40)).tobytes() == np.delete(lap[7], (7, 40)).tobytes() and lap[40, 7] == lap[7, 40]
    sc.check(y, 0, 70, metric, sc.oracle(y, metric), deg=deg, a=a, lap=lap, label='hip identical points %s %s' % (metric, dt.name))
  far = np.array(sc.case(70, 3, dt, seed=2))
  far[69] = 1000.0                                        # every 'rbf' affinity to it underflows: exp(-3e6) = 0
  deg, _, a, lap = _pipeline(be, far, 0, 70, 'rbf')
  assert deg[69] == 1 and a[69, 69] == 1 and not np.any(a[69, :69]) and not np.any(a[:69, 69])
  assert lap[69, 69] == 1 and not np.any(lap[69, :69]) and np.all(np.isfinite(lap))
  near = sc.oracle(far[:69], 'rbf')                       # the other 69 points see nothing of it
  sc.check(far[:69], 0, 69, 'rbf', near, deg=deg[:69], a=a[:69, :69], lap=lap[:69, :69], label='hip far point %s' % dt.name)
  one = np.array([[0.25, -3.0]], dt)
  deg, _, a, lap = _pipeline(be, one, 0, 1, 'euclidean')
  assert deg.tolist() == [0.0] and sc.scale_of(deg).tolist() == [1.0] and a.tolist() == [[0.0]] and lap.tolist() == [[1.0]]


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_gamma_and_empty_shapes(be, dtype):
  dt = np.dtype(dtype)
  y = sc.case(66, 4, dt, seed=3)
  yt = be.from_numpy(y)
  for gamma in (0.5, 2.0):
    want = sc.oracle(y, 'rbf', gamma)
    deg = be.affinity_degree(yt, yt, 'rbf', gamma).numpy()
    a = be.affinity_matrix(yt, 0, yt, 'rbf', gamma).numpy()
    sc.check(y, 0, 66, 'rbf', want, deg=deg, a=a, label='hip gamma=%g %s' % (gamma, dt.name))
  before = be.launches
  for metric in sc.METRICS:
    assert be.affinity_degree(be.from_numpy(y[:0]), yt, metric, 1.0).numpy().shape == (0,)
    assert be.affinity_matrix(be.from_numpy(y[:0]), 0, yt, metric, 1.0).numpy().shape == (0, 66)
  assert be.launches == before                            # m = 0: nothing is launched
  for metric in sc.METRICS:
    none = be.from_numpy(np.zeros((0, 4), dt))
    assert not np.any(be.affinity_degree(yt, none, metric, 1.0).numpy())          # n = 0: D = 0
    flat = be.from_numpy(np.zeros((5, 0), dt))                                    # d = 0: every distance is 0
    assert np.all(be.affinity_degree(flat, flat, metric, 1.0).numpy() == (5 if metric == 'rbf' else 0))
    assert np.all(be.affinity_matrix(flat, 0, flat, metric, 1.0).numpy() == (1 if metric == 'rbf' else 0))


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('pad', (3, 4))
def test_views_of_wider_buffers_give_the_same_bits(be, pad, dtype):
  dt = np.dtype(dtype)
  n, d, r0, m = 130, 5, 60, 67
  y = sc.case(n, d, dt, seed=1)
  deg, deg_all, a, lap = _pipeline(be, y, r0, m, 'rbf')
  scale = sc.scale_of(deg_all)
  (xt, xbuf, xframe), (yt, ybuf, yframe) = _framed(be, np.ascontiguousarray(y[r0:r0 + m]), 3), _framed(be, y, 5)
  # pad = 4: rows 136 elements apart, a multiple of 16 bytes (the vector stores' condition on ldo), behind a pointer
  # that is not aligned; pad = 3: 135 elements, which in float32 is not
  (ot, obuf, oframe), (lt, lbuf, lframe) = _framed(be, np.zeros((m, n), dt), pad + 2), _framed(be, np.zeros((m, n), dt), pad + 2)
  dt_out = be.empty((m,), dt)
  kernels.affinity_degree(xt, yt, 'rbf', 1.0, dt_out)
  kernels.affinity_matrix(xt, r0, yt, 'rbf', 1.0, ot)
  kernels.affinity_matrix(xt, r0, yt, 'rbf', 1.0, lt, scale=be.from_numpy(scale))
  assert dt_out.numpy().tobytes() == deg.tobytes()
  assert ot.numpy().tobytes() == a.tobytes() and lt.numpy().tobytes() == lap.tobytes()
  assert xbuf.numpy().tobytes() == xframe.tobytes() and ybuf.numpy().tobytes() == yframe.tobytes()     # inputs unchanged
  oframe[1:m + 1, 1:n + 1] = a
  lframe[1:m + 1, 1:n + 1] = lap
  assert obuf.numpy().tobytes() == oframe.tobytes() and lbuf.numpy().tobytes() == lframe.tobytes()     # frames untouched
  # an aligned target whose rows are a multiple of four elements apart (the vector stores), inside a wider buffer
  wide = be.from_numpy(np.full((m, n + 10), -77.0, dt))
  kernels.affinity_matrix(xt, r0, yt, 'rbf', 1.0, wide[:, :n], scale=be.from_numpy(scale))
  got = wide.numpy()
  assert got[:, :n].tobytes() == lap.tobytes() and np.all(got[:, n:] == -77.0)


def test_refusals_launch_nothing(be):
  y = sc.case(9, 3, np.dtype(np.float32))
  yt = be.from_numpy(y)
  before = be.launches
  for bad in (y.astype(np.int32), y.astype(np.float16)):
    with pytest.raises(TypeError, match='astype'):
      be.affinity_degree(be.from_numpy(bad), be.from_numpy(bad))
    with pytest.raises(TypeError, match='astype'):
      be.affinity_matrix(be.from_numpy(bad), 0, be.from_numpy(bad))
  with pytest.raises(TypeError, match='astype'):
    be.affinity_degree(yt, be.from_numpy(y.astype(np.float64)))
  with pytest.raises(TypeError, match='astype'):
    be.affinity_matrix(yt, 0, yt, scale=be.from_numpy(np.ones(9, np.float64)))
  for call in (lambda **kw: be.affinity_degree(yt, yt, **kw), lambda **kw: be.affinity_matrix(yt, 0, yt, **kw)):
    with pytest.raises(NotImplementedError, match='np.square'):
      call(metric='scaled_euclidean')
    with pytest.raises(ValueError, match='unknown metric'):
      call(metric='cosine')
    for gamma in (float('nan'), float('inf'), float('-inf')):
      with pytest.raises(ValueError, match='gamma'):
        call(gamma=gamma)
  with pytest.raises(ValueError, match='fit'):
    be.affinity_degree(yt, be.from_numpy(np.zeros((4, 2), np.float32)))
  for r0, rows in ((-1, 3), (7, 3), (1, 9)):
    with pytest.raises(ValueError, match='not among'):
      be.affinity_matrix(be.from_numpy(y[:rows]), r0, yt)
  with pytest.raises(ValueError, match='scale of shape'):
    be.affinity_matrix(yt, 0, yt, scale=be.from_numpy(np.ones(8, np.float32)))
  with pytest.raises(ValueError, match='target'):
    kernels.affinity_degree(yt, yt, 'rbf', 1.0, be.empty((8,), np.float32))
  with pytest.raises(ValueError, match='target of shape'):
    kernels.affinity_matrix(yt, 0, yt, 'rbf', 1.0, be.empty((9, 8), np.float32))
  with pytest.raises(TypeError, match='astype'):
    kernels.affinity_matrix(yt, 0, yt, 'rbf', 1.0, be.empty((9, 9), np.float64))
  assert be.launches == before
  # the library's own refusals
  lib, err = _hip.extras(), _hip.lib().sp_last_error
  f32 = _hip.SP_F32

  def degree(dtype=f32, metric=0, gamma=1.0, ldx=3, m=9, ldy=3, n=9, d=3, ws_bytes=0):
    return lib.sp_affinity_degree(dtype, metric, gamma, None, ldx, m, None, ldy, n, d, None, None, ws_bytes, None)

  def matrix(dtype=f32, metric=0, gamma=1.0, ldx=3, m=9, r0=0, ldy=3, n=9, d=3, ldo=9):
    return lib.sp_affinity_matrix(dtype, metric, gamma, None, ldx, m, r0, None, ldy, n, d, None, None, ldo, None)

  for fn in (degree, matrix):
    for dtype in (_hip.SP_I32, _hip.SP_F16):
      assert fn(dtype=dtype) != 0 and 'astype' in err().decode()
    for metric in (-1, 3):
      assert fn(metric=metric) != 0 and 'unknown metric' in err().decode()
    for gamma in (float('nan'), float('inf'), 1e300):        # (1e300 is not finite in float32)
      assert fn(gamma=gamma) != 0 and 'gamma' in err().decode()
    assert fn(ldx=2) != 0 and 'bad shape' in err().decode()
    assert fn(ldy=2) != 0 and 'bad shape' in err().decode()
    assert fn() != 0 and 'required' in err().decode()        # (no operands: refused before anything is launched)
  for r0, m in ((-1, 3), (7, 3), (1, 9)):
    assert matrix(r0=r0, m=m) != 0 and 'not among' in err().decode()
  assert matrix(ldo=8) != 0 and 'ldo' in err().decode()
  # a workspace that is too small: n = 449 needs two ranges of m partial degrees
  need = lib.sp_affinity_degree_workspace_bytes(f32, 9, 449, 3)
  assert need == 2 * 9 * 4 and lib.sp_affinity_degree_workspace_bytes(f32, 9, 448, 3) == 0
  big = be.from_numpy(sc.case(449, 3, np.dtype(np.float32)))
  out, ws = be.empty((9,), np.float32), be.empty((need,), np.uint8)
  before = be.launches
  rc = lib.sp_affinity_degree(f32, 0, 1.0, yt.data_ptr(), 3, 9, big.data_ptr(), 3, 449, 3, out.data_ptr(), ws.data_ptr(),
                              need - 1, None)
  assert rc != 0 and 'workspace' in err().decode()
  rc = lib.sp_affinity_degree(f32, 0, 1.0, yt.data_ptr(), 3, 9, big.data_ptr(), 3, 449, 3, out.data_ptr(), None, 0, None)
  assert rc != 0 and 'workspace' in err().decode()


# ---- the driver on the device -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('workers', (1, 4))
def test_the_driver_finds_the_planted_groups_gpu(workers, dtype):
  # Ritz values within 2 (e_L + n u): the n u term is for the matrix-vector product in the run's dtype
  ex.check_driver('hip', workers, dtype, extra=2 * 60 * sc.U[np.dtype(dtype)])


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_laplacian_does_not_depend_on_the_workers_gpu(dtype):
  ex.check_laplacian_bits('hip', dtype)


def test_driver_refusals_gpu():
  ex.check_refusals('hip')
