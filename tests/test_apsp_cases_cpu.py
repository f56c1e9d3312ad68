"""What the shortest-path tests stand on, without a GPU: the NumPy bodies of the Isomap driver (examples/sklearn/
manifold/_graph.py) against the oracle and the derived bound of tests/apsp_cases.py, and the agreement of header,
binding and library."""
import ctypes
import os

import numpy as np
import pytest

from spartan_amd import _hip
from tests import apsp_cases as ac

DTYPES = (np.float32, np.float64)
SIZES = (0, 1, 2, 63, 65, 200)


@pytest.fixture(scope='module')
def graph():
  import spartan_amd as sp
  from oracle.np_backend import NumpyBackend
  from spartan_amd.examples.sklearn.manifold import _graph
  sp.initialize(backend=NumpyBackend(), num_workers=1)
  yield _graph
  sp.shutdown()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n', SIZES)
def test_numpy_apsp_matches_the_oracle(graph, n, dtype):
  for w in (ac.integer_graph(n, 4, dtype), ac.permuted_chain(n, dtype)):
    before = w.copy()
    ac.check_exact(graph.apsp(w), w)
    assert w.tobytes() == before.tobytes()
  w = ac.real_graph(n, 4, dtype)
  ac.check_real(graph.apsp(w), w, label='numpy')


def test_numpy_apsp_refusals(graph):
  w = ac.real_graph(9, 3, np.float64)
  for bad in (-1.0, np.nan):
    v = w.copy()
    v[2, 5] = bad
    with pytest.raises(ValueError, match='negative or NaN'):
      graph.apsp(v)
  v = w.copy()
  v[3, 3] = -4.0                             # the diagonal is ignored
  ac.check_real(graph.apsp(v), w, label='numpy')
  with pytest.raises(TypeError, match='astype'):
    graph.apsp(np.ones((4, 4), np.int32))
  with pytest.raises(ValueError, match='square'):
    graph.apsp(w[:4])


def test_numpy_graph_from_knn(graph):
  dist = np.array([[1.0, 2.0, 9.0], [3.0, 0.5, 9.0], [4.0, 7.0, 9.0], [6.0, 9.0, 9.0]])
  idx = np.array([[1, 2, -1], [0, 2, -1], [0, 3, -3], [3, 7, -1]], np.int64)       # (3 lists itself and a row out of range)
  w = graph.graph_from_knn(dist, idx)
  inf = np.inf
  want = np.array([[0, 1.0, 2.0, inf], [1.0, 0, 0.5, inf], [2.0, 0.5, 0, 7.0], [inf, inf, 7.0, 0]])
  np.testing.assert_array_equal(w, want)
  assert graph.graph_from_knn(dist.astype(np.float32), idx).dtype == np.float32
  assert graph.graph_from_knn(np.zeros((1, 1)), np.zeros((1, 1), np.int64)).tolist() == [[0.0]]
  with pytest.raises(TypeError):
    graph.graph_from_knn(dist, idx.astype(np.int32))
  with pytest.raises(ValueError):
    graph.graph_from_knn(dist, idx[:, :2])


def test_the_graph_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  names = _declared_functions(os.path.join(ROOT, 'include', 'spartan_hip_graph.h'))
  assert names == sorted(_hip.EXPORTS_GRAPH) == ['sp_apsp', 'sp_graph_from_knn']
  others = set(_declared_functions(EXTRAS_HEADER)) | set(_hip.EXPORTS) | set(_hip.EXPORTS_EIG) | set(_hip.EXPORTS_KNN)
  assert not set(names) & others
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  x = _hip.extras()                                   # host code: the refusals need no device
  assert x.sp_apsp(_hip.SP_I32, None, 4, 4, None, None) != 0
  assert 'astype' in _hip.lib().sp_last_error().decode()
  assert x.sp_apsp(_hip.SP_F32, None, 3, 4, None, None) != 0          # ldd < n
  assert x.sp_graph_from_knn(_hip.SP_F16, None, None, 2, 4, 2, None, 4, None) != 0
  assert 'astype' in _hip.lib().sp_last_error().decode()
  assert x.sp_graph_from_knn(_hip.SP_F64, None, None, 1, 4, 2, None, 4, None) != 0      # ldk < k
