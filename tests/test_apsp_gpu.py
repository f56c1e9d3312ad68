"""sp_apsp / sp_graph_from_knn (csrc/apsp.hip) through HipBackend.apsp / graph_from_knn and through kernels.apsp, against
the oracle and the derived bound of tests/apsp_cases.py.

Sizes: the kernel works in blocks of 64 -- n on both sides of one, two and three blocks (63, 64, 65, 127, 128, 129), 200
(four blocks, the last one ragged) and 0, 1, 2.  Measured figures are printed before each assertion (pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import kernels
from spartan_amd.examples.sklearn.manifold import _graph
from tests import apsp_cases as ac

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)


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


def _apsp(be, w):
  t = be.from_numpy(w)
  before = be.launches
  out = be.apsp(t)
  assert be.launches - before == (1 if w.shape[0] else 0)
  assert t.numpy().tobytes() == w.tobytes()                  # the input is never written
  return out.numpy()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', SIZES)
def test_integer_graphs_match_the_oracle_bit_for_bit(be, n, dtype):
  w = ac.integer_graph(n, 4, dtype)
  ac.check_exact(_apsp(be, w), w)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', SIZES)
def test_permuted_chains_match_the_oracle_bit_for_bit(be, n, dtype):
  w = ac.permuted_chain(n, dtype)
  got = _apsp(be, w)
  ac.check_exact(got, w)
  assert np.all(np.isfinite(got))


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', SIZES)
def test_real_graphs_meet_the_derived_bound(be, n, dtype):
  w = ac.real_graph(n, 4, dtype)
  ac.check_real(_apsp(be, w), w, label='hip')


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', (65, 200))
def test_a_row_view_of_a_wider_buffer_and_its_frame(be, n, dtype):
  """ldd > n: in place through kernels.apsp, only the n x n box changes; through HipBackend.apsp nothing changes."""
  w = ac.integer_graph(n, 4, dtype, seed=1)
  view, buf, frame = _framed(be, w, 5)
  out = be.apsp(view)
  ac.check_exact(out.numpy(), w)
  assert buf.numpy().tobytes() == frame.tobytes()
  info = be.empty((1,), np.int32)
  kernels.apsp(view, info)
  assert int(info.numpy()[0]) == 0
  after = buf.numpy()
  ac.check_exact(np.ascontiguousarray(after[1:n + 1, 1:n + 1]), w)
  after[1:n + 1, 1:n + 1] = w
  assert after.tobytes() == frame.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', (129, 200))
def test_a_symmetric_input_gives_a_bit_symmetric_output(be, n, dtype):
  w = ac.real_graph(n, 4, dtype, seed=2)
  w = np.minimum(w, w.T)
  got = _apsp(be, w)
  ac.check_real(got, w, label='hip symmetric')
  assert got.tobytes() == np.ascontiguousarray(got.T).tobytes()


def test_refusals(be):
  w = ac.real_graph(70, 3, np.float32)
  for bad in (-1.0, np.nan):
    v = w.copy()
    v[2, 69] = bad
    with pytest.raises(ValueError, match='negative or NaN'):
      be.apsp(be.from_numpy(v))
  v = w.copy()
  v[3, 3] = -4.0                             # the diagonal is ignored
  v[69, 69] = np.nan
  ac.check_real(be.apsp(be.from_numpy(v)).numpy(), w, label='hip diagonal')
  before = be.launches
  for dt in (np.int32, np.float16):
    with pytest.raises(TypeError, match='astype'):
      be.apsp(be.from_numpy(np.ones((4, 4), dt)))
    with pytest.raises(TypeError, match='astype'):
      be.graph_from_knn(be.from_numpy(np.ones((4, 2), dt)), be.from_numpy(np.zeros((4, 2), np.int64)))
  with pytest.raises(ValueError, match='square'):
    be.apsp(be.from_numpy(w[:4]))
  with pytest.raises(TypeError, match='int64'):
    be.graph_from_knn(be.from_numpy(np.ones((4, 2), np.float32)), be.from_numpy(np.zeros((4, 2), np.int32)))
  with pytest.raises(ValueError):
    be.graph_from_knn(be.from_numpy(np.ones((4, 2), np.float32)), be.from_numpy(np.zeros((4, 3), np.int64)))
  assert be.launches == before


def _lists(n, k, dtype, seed):
  """Neighbour lists with padding, rows that list themselves, and pairs stated in both directions with two weights."""
  rng = np.random.RandomState(seed)
  idx = rng.randint(0, n, size=(n, k)).astype(np.int64)
  dist = rng.uniform(0.5, 2.0, size=(n, k)).astype(dtype)
  idx[rng.rand(n, k) < 0.2] = -1
  return dist, idx


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_graph_from_knn_matches_the_numpy_body(be, dtype):
  cases = [_lists(70, 5, dtype, 1), _lists(9, 1, dtype, 2), _lists(1, 1, dtype, 3), _lists(1, 3, dtype, 4),
           _lists(130, 9, dtype, 5)]
  # a pair listed in both directions with two different weights: the smaller wins on both sides
  dist = np.array([[3.0, 1.5], [2.0, 4.0], [0.25, 8.0]], dtype)
  idx = np.array([[1, 2], [0, -1], [0, 1]], np.int64)
  cases.append((dist, idx))
  for dist, idx in cases:
    want = _graph.graph_from_knn_numpy(dist, idx)
    before = be.launches
    got = be.graph_from_knn(be.from_numpy(dist), be.from_numpy(idx)).numpy()
    assert be.launches - before == 1
    assert got.dtype == np.dtype(dtype) and got.tobytes() == want.tobytes()
    # the lists as row views of wider arrays (one row stride for both)
    (dv, dbuf, dframe), (iv, ibuf, iframe) = _framed(be, dist, 4), _framed(be, idx, 4, fill=-5)
    assert be.graph_from_knn(dv, iv).numpy().tobytes() == want.tobytes()
    assert dbuf.numpy().tobytes() == dframe.tobytes() and ibuf.numpy().tobytes() == iframe.tobytes()
  got = be.graph_from_knn(be.from_numpy(dist), be.from_numpy(idx)).numpy()
  assert got[0, 1] == got[1, 0] == 2.0 and got[0, 2] == got[2, 0] == 0.25 and got[1, 2] == got[2, 1] == 8.0


def test_graph_then_apsp(be):
  """The two kernels in a row, as the Isomap driver calls them."""
  dist, idx = _lists(130, 4, np.float32, 6)
  w = _graph.graph_from_knn_numpy(dist, idx)
  got = be.apsp(be.graph_from_knn(be.from_numpy(dist), be.from_numpy(idx))).numpy()
  ac.check_real(got, w, label='hip from lists')
  assert got.tobytes() == np.ascontiguousarray(got.T).tobytes()
