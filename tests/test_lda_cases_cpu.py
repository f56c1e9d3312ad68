"""What the LDA tests stand on, without a GPU: the two-product form of the driver's NumPy tile body
(examples/_lda.step_numpy) against the oracle and the derived bound of tests/lda_cases.py, the empty document and the
absent term, the refusals of check_params, and the agreement of header, binding and library."""
import ctypes
import os

import numpy as np
import pytest

from spartan_amd import _hip
from tests import lda_cases as lc

DTYPES = (np.float32, np.float64)
# (V, D, k, iters): the shapes at which the two-product form was checked against the reference's loops
SHAPES = ((160, 200, 16, 1), (160, 200, 16, 3), (70, 130, 33, 2), (257, 65, 128, 2))


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d-i%d' % s)
def test_the_numpy_tile_body_meets_the_bound_at_the_shapes_of_its_derivation(shape, dtype):
  from spartan_amd.examples import _lda
  v, d, k, iters = shape
  x, n = lc.case(v, d, k, np.dtype(dtype))
  want = lc.oracle_of_case(v, d, k, np.dtype(dtype), iters)
  delta, doc_topics = _lda.step_numpy(x, n, lc.ALPHA, lc.ETA, iters)
  share = lc.check_step(x, n, lc.ALPHA, lc.ETA, iters, delta, doc_topics, want=want,
                        label='numpy body %s %s' % (shape, np.dtype(dtype).name))
  assert max(share.values()) <= 0.5      # (more would mean that the derivation is wrong, not that the tolerance is tight)
  assert np.all(np.isnan(doc_topics[7])) and not np.any(delta[:, 11])
  ok = ~np.isnan(doc_topics).any(axis=1)
  assert np.all(np.abs(doc_topics[ok].sum(axis=1) - 1) <= 4 * k * np.finfo(dtype).eps)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_signed_counts_meet_the_bound_relative_to_the_absolute_sum(dtype):
  from spartan_amd.examples import _lda
  v, d, k, iters = 70, 130, 33, 2
  x, n = lc.case(v, d, k, np.dtype(dtype), signed=True)
  assert np.any(x < 0) and np.any(x > 0)
  delta, doc_topics = _lda.step_numpy(x, n, lc.ALPHA, lc.ETA, iters)
  lc.check_step(x, n, lc.ALPHA, lc.ETA, iters, delta, doc_topics,
                want=lc.oracle_of_case(v, d, k, np.dtype(dtype), iters, signed=True), label='numpy body, signed counts')
  # |x| in c: the documents' topics are those of the absolute counts
  assert _lda.step_numpy(np.abs(x), n, lc.ALPHA, lc.ETA, iters)[1].tobytes() == doc_topics.tobytes()


@pytest.mark.parametrize('iters', (1, 2, 3))
def test_an_empty_document_is_nan_and_adds_exactly_nothing(iters):
  from spartan_amd.examples import _lda
  x, n = lc.case(70, 20, 5, np.dtype(np.float64))
  assert not np.any(x[:, 7])
  delta, doc_topics = _lda.step_numpy(x, n, lc.ALPHA, lc.ETA, iters)
  without = np.delete(x, 7, axis=1)
  delta2, doc_topics2 = _lda.step_numpy(without, n, lc.ALPHA, lc.ETA, iters)
  assert np.all(np.isnan(doc_topics[7])) and not np.isnan(np.delete(doc_topics, 7, axis=0)).any()
  assert np.all(np.isfinite(delta))
  np.testing.assert_allclose(delta, delta2, rtol=1e-13, atol=0)       # (another D: NumPy may add in another order)
  np.testing.assert_allclose(np.delete(doc_topics, 7, axis=0), doc_topics2, rtol=1e-13, atol=0)
  # all documents empty, no document, no term
  delta, doc_topics = _lda.step_numpy(np.zeros((70, 3)), n, lc.ALPHA, lc.ETA, iters)
  assert delta.shape == (5, 70) and not np.any(delta) and np.all(np.isnan(doc_topics))
  delta, doc_topics = _lda.step_numpy(np.zeros((70, 0)), n, lc.ALPHA, lc.ETA, iters)
  assert delta.shape == (5, 70) and not np.any(delta) and doc_topics.shape == (0, 5)
  delta, doc_topics = _lda.step_numpy(np.zeros((0, 4)), n[:, :0], lc.ALPHA, lc.ETA, iters)
  assert delta.shape == (5, 0) and doc_topics.shape == (4, 5) and np.all(np.isnan(doc_topics))


def test_the_oracle_is_the_reference_loop():
  """The oracle against a word-for-word float64 transcription of the reference's loops (lda.py:22-50) on a small case."""
  x, n = lc.case(30, 12, 4, np.dtype(np.float64))
  iters, alpha, eta = 2, lc.ALPHA, lc.ETA
  k, v = n.shape
  ts = np.linalg.norm(n, 1, axis=1)
  local = n.copy()
  doc_topics = np.zeros((x.shape[1], k))
  with np.errstate(all='ignore'):
    for doc_id in range(x.shape[1]):
      doc = x[:, doc_id]
      gamma = np.ones(k) / k
      model = np.zeros((k, v))
      for _ in range(iters):
        for j in doc.nonzero()[0]:
          model[:, j] = (n[:, j] + eta) * (gamma + alpha) / (ts + eta * doc.shape[0])
        for j in model[0].nonzero()[0]:
          model[:, j] /= model[:, j].sum()
        for j in doc.nonzero()[0]:
          model[:, j] *= doc[j]
        gamma = np.linalg.norm(model, 1, axis=1)
        gamma = gamma / np.linalg.norm(gamma, 1)
      local += model
      doc_topics[doc_id] = gamma
  want = lc.oracle(x, n, alpha, eta, iters)
  np.testing.assert_allclose(local - n, want['delta'].astype(np.float64), rtol=1e-12, atol=1e-15)
  np.testing.assert_allclose(doc_topics, want['doc_topics'].astype(np.float64), rtol=1e-12, atol=0)


def test_check_params_refuses_what_the_kernel_refuses():
  from spartan_amd.examples import _lda
  assert _lda.check_params(5, 0.1, 0.2, 3) == (5, 0.1, 0.2, 3) and _hip.SP_LDA_MAX_K == 128
  assert _lda.check_params(128, 1e-300, 1e300, 1)[0] == 128
  for k in (0, -1, 129):
    with pytest.raises(ValueError, match='k = '):
      _lda.check_params(k, 0.1, 0.1, 1)
  for iters in (0, -2):
    with pytest.raises(ValueError, match='iters = '):
      _lda.check_params(5, 0.1, 0.1, iters)
  for bad in (0.0, -0.1, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='alpha = '):
      _lda.check_params(5, bad, 0.1, 1)
    with pytest.raises(ValueError, match='eta = '):
      _lda.check_params(5, 0.1, bad, 1)


def test_the_lda_header_the_binding_and_the_library_agree():
  from tests.test_abi_cpu import EXTRAS_HEADER, ROOT, _declared_functions
  header = os.path.join(ROOT, 'include', 'spartan_hip_lda.h')
  names = _declared_functions(header)
  assert names == sorted(_hip.EXPORTS_LDA) == ['sp_lda_step', 'sp_lda_step_workspace_bytes']
  others = (set(_hip.EXPORTS) | set(_hip.EXPORTS_EXTRAS) | set(_hip.EXPORTS_EIG) | set(_hip.EXPORTS_KNN)
            | set(_hip.EXPORTS_GRAPH) | set(_hip.EXPORTS_ALS) | set(_hip.EXPORTS_FUZZY))
  for h in (EXTRAS_HEADER,) + tuple(os.path.join(ROOT, 'include', 'spartan_hip_%s.h' % s)
                                    for s in ('eig', 'knn', 'graph', 'als', 'fuzzy')):
    others |= set(_declared_functions(h))
  assert not set(names) & others
  text = open(header).read()
  assert '#define SP_LDA_MAX_K %d' % _hip.SP_LDA_MAX_K in text
  xraw = ctypes.CDLL(_hip.EXTRAS_LIB_PATH)
  assert not [n for n in names if not hasattr(xraw, n)]
  assert not [n for n in names if hasattr(ctypes.CDLL(_hip.LIB_PATH), n)]
  x = _hip.extras()                                   # host code: sizes need no device
  f32, f64 = _hip.SP_F32, _hip.SP_F64
  size = x.sp_lda_step_workspace_bytes
  # A [V][KP] and the stored B [D][KP], each rounded up to 256 bytes; KP = 16, 32, 64, 128
  assert size(f32, 160, 64, 16, 1, 0) == 160 * 16 * 4 + 64 * 16 * 4 == size(f32, 160, 64, 1, 3, 5)
  assert size(f64, 160, 64, 17, 1, 0) == 160 * 32 * 8 + 64 * 32 * 8
  assert size(f64, 10, 10, 128, 1, 0) == 2 * 10 * 128 * 8 == size(f64, 10, 10, 65, 1, 0)
  assert size(f32, 0, 0, 5, 1, 0) == 512                                        # never 0 for arguments that are taken
  partials = -(-3 * 33 * 70 * 8 // 256) * 256                                  # three partial [k, V]
  assert size(f64, 70, 200, 33, 2, 3) == 70 * 64 * 8 + 200 * 64 * 8 + partials
  assert size(f64, 70, 200, 33, 2, 9) == size(f64, 70, 200, 33, 2, 4)          # at most ceil(200 / 64) = 4 ranges
  assert size(f64, 70, 200, 33, 2, 0) == size(f64, 70, 200, 33, 2, 4)          # two blocks of terms: every block a range
  assert (size(_hip.SP_I32, 70, 200, 33, 2, 0) == 0 == size(f32, 70, 200, 0, 2, 0) == size(f32, 70, 200, 129, 2, 0)
          == size(f32, -1, 4, 4, 1, 0) == size(f32, 4, 4, 4, 0, 0) == size(f32, 4, 4, 4, 1, -1))
