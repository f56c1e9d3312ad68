"""Latent Dirichlet allocation by collapsed variational Bayes, CVB0 (interface of the reference's
spartan/examples/lda.py: `learn_topics(terms_docs_matrix, k_topics, alpha, eta, max_iter, max_iter_per_doc)` ->
(doc_topics, topic_term_counts), expressions of shape (D, k) and (k, V)).

The structure is the reference's.  X [V, D] holds the count of every term in every document, N [k, V] the topic / term
counts; `max_iter` times
  N = outer((X, N), (1, None), fn=_train_mapper, reducer=np.add)
in which a tile body gets ALL terms of a band of documents and the whole N and yields N + delta; then one
  doc_topics = outer((X, N), (1, None), fn=_doc_topic_mapper)
for the inference; last, the rows of N are divided by their sums of absolute values (reduce and map kernels).  The
reference's body is a Python triple loop over documents, inner iterations and non-zero terms; here it is one call of
_lda.lda_step per band (HipBackend: sp_lda_step -- the loops fused into two small matrix products around a quotient,
nothing of size V x D or k x V per document is written).  Per document (lda.py:22-50):

    gamma_t = 1 / k;  `max_iter_per_doc` times:
      p_tj = (N_tj + eta) (gamma_t + alpha) / (sum_j |N_tj| + eta V),  q_tj = x_j p_tj / sum_t p_tj  (terms with x_j != 0)
      gamma_t = sum_j |q_tj| / sum_tj |q_tj|
    doc_topics[d] = gamma;  delta += q of the last iteration

Behaviour of the reference that is kept because its recorded outputs (tests/golden/lda_w4.npz) are the yardstick:
EVERY document tile yields N + delta and the tiles' results are added, so with T tiles of documents an iteration gives
T . N + sum of the deltas, not N + sum of the deltas; the result of training depends on the tiling.  A document without
a term gets a row of NaN in doc_topics (0 / 0) and adds nothing to the counts.

Additions: `topic_term_counts` is the start (a NumPy array or an expression of shape (k, V); default: the reference's
expr.rand); `dtype` is float32 or float64 (default: the matrix's own if it is one of the two, else float64 -- integer
counts such as expr.randint's are converted on the device).  ValueError for k_topics outside 1 .. 128,
max_iter_per_doc < 1, alpha or eta that is not finite and > 0 (with either not > 0 the reference's test for "non-zero
term" fails silently), max_iter < 0 and a matrix that is not 2-D."""
import numpy as np

from .. import context, expr, tile_checks
from ..array import distarray, extent
from . import _lda

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _tile_in(tile, dtype):
  return tile if isinstance(tile, distarray.Absent) else context.get().backend.astype(tile, dtype)


def _train_mapper(ex_a, terms_docs, ex_b, counts, alpha=None, eta=None, iters=None, dtype=None):
  """Tile body of a training iteration: N + delta of this band of documents (lda.py:56-80)."""
  terms_docs, counts = _tile_in(terms_docs, dtype), _tile_in(counts, dtype)
  delta, _ = _lda.lda_step(terms_docs, counts, alpha, eta, iters, want_doc_topics=False)
  shape = (counts.shape[0], ex_a.array_shape[0])
  yield extent.create((0, 0), shape, shape), (delta if isinstance(delta, distarray.Absent) else counts + delta)


def _doc_topic_mapper(ex_a, terms_docs, ex_b, counts, alpha=None, eta=None, iters=None, dtype=None):
  """Tile body of the inference: the rows of doc_topics of this band of documents (lda.py:84-110)."""
  terms_docs, counts = _tile_in(terms_docs, dtype), _tile_in(counts, dtype)
  _, doc_topics = _lda.lda_step(terms_docs, counts, alpha, eta, iters, want_delta=False)
  k = counts.shape[0]
  yield extent.create((ex_a.ul[1], 0), (ex_a.lr[1], k), (ex_a.array_shape[1], k)), doc_topics


_train_mapper.yields_fresh_tensors = True      # the kernel's output (or NumPy's) or a new sum, never a fetched tile
_doc_topic_mapper.yields_fresh_tensors = True


def learn_topics(terms_docs_matrix, k_topics, alpha=0.1, eta=0.1, max_iter=10, max_iter_per_doc=1,
                 topic_term_counts=None, dtype=None):
  """(doc_topics [D, k], topic_term_counts [k, V]), expressions in `dtype`, after `max_iter` training iterations and
  one inference on `terms_docs_matrix` [V, D] (expression / distributed array / NumPy array), every document renewed
  `max_iter_per_doc` times per pass.  The returned counts have rows of unit 1-norm.  See the module docstring for the
  reference's behaviour that is kept (every document tile adds its own copy of the counts) and for the additions."""
  k_topics, alpha, eta, max_iter_per_doc = _lda.check_params(k_topics, alpha, eta, max_iter_per_doc, 'learn_topics')
  max_iter = int(max_iter)
  if max_iter < 0:
    raise ValueError('learn_topics: max_iter = %d' % max_iter)
  if isinstance(terms_docs_matrix, np.ndarray):
    terms_docs_matrix = expr.from_numpy(terms_docs_matrix)
  if len(terms_docs_matrix.shape) != 2:
    raise ValueError('learn_topics: expected a terms x documents matrix, got shape %s' % (tuple(terms_docs_matrix.shape),))
  num_terms, num_docs = (int(v) for v in terms_docs_matrix.shape)
  if hasattr(terms_docs_matrix, 'evaluate'):
    terms_docs_matrix = terms_docs_matrix.evaluate()      # (every pass reads it; its dtype decides the run's)
  if dtype is None:
    own = np.dtype(terms_docs_matrix.dtype)
    dtype = own if own in _FLOATS else np.dtype(np.float64)
  dtype = tile_checks.check_float_dtype(dtype, 'learn_topics')
  if topic_term_counts is None:
    topic_term_counts = expr.rand(k_topics, num_terms)
  elif isinstance(topic_term_counts, np.ndarray):
    topic_term_counts = expr.from_numpy(topic_term_counts)
  if tuple(topic_term_counts.shape) != (k_topics, num_terms):
    raise ValueError('learn_topics: topic_term_counts of shape %s for %d topics and %d terms'
                     % (tuple(topic_term_counts.shape), k_topics, num_terms))
  kw = {'alpha': alpha, 'eta': eta, 'iters': max_iter_per_doc, 'dtype': dtype}
  for _ in range(max_iter):
    topic_term_counts = expr.outer((terms_docs_matrix, topic_term_counts), (1, None), fn=_train_mapper, fn_kw=kw,
                                   shape=(k_topics, num_terms), dtype=dtype, reducer=np.add)
  doc_topics = expr.outer((terms_docs_matrix, topic_term_counts), (1, None), fn=_doc_topic_mapper, fn_kw=kw,
                          shape=(num_docs, k_topics), dtype=dtype)
  # the rows of the counts, divided by their sums of absolute values
  norm_val = expr.sum(expr.abs(topic_term_counts), axis=1)
  topic_term_counts = topic_term_counts / expr.reshape(norm_val, (k_topics, 1))
  return doc_topics, topic_term_counts
