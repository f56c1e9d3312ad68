"""The tile body of the LDA driver: backend.lda_step where the backend has it (HipBackend: sp_lda_step), NumPy on host
arrays otherwise -- the same two-product form in the tile's dtype (include/spartan_hip_lda.h), which keeps the driver
runnable on a backend of plain NumPy tiles."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray

check_params = tile_checks.check_lda_params      # (the driver checks its own parameters with it)


def step_numpy(x, n, alpha, eta, iters):
  """(delta [k, V], doc_topics [D, k]) in the dtype of x [V, D] and n [k, V]: the kernel's form.  With
  A = (n + eta) / (sum_j |n| + eta V), B = gamma + alpha, S = A^T B^T and W = x / S where x != 0 (0 otherwise):
  c = B o (|W|^T |A|^T), gamma = c / sum_t c, `iters` times from gamma = 1 / k; delta = A o (B^T W^T) with the B that
  entered the last iteration, the rows of empty documents (whose gamma is NaN) taken as 0.  The sums are NumPy's, in
  another order than the kernel's."""
  dt = x.dtype
  v, d = x.shape
  k = n.shape[0]
  alpha, eta = dt.type(alpha), dt.type(eta)
  with np.errstate(all='ignore'):
    den = np.abs(n).sum(axis=1) + eta * dt.type(v)
    a = (n + eta) / den[:, None]                                   # [k, V]
    nz = x != 0
    empty = ~nz.any(axis=0)                                        # [D]
    gamma = np.full((d, k), dt.type(1) / dt.type(k), dt)
    for _ in range(iters):
      b = gamma + alpha                                            # [D, k]
      s = a.T.dot(b.T)                                             # [V, D]
      w = np.zeros((v, d), dt)
      np.divide(x, s, out=w, where=nz)
      c = b * np.abs(w).T.dot(np.abs(a).T)
      gamma = c / c.sum(axis=1)[:, None]
    b = np.where(empty[:, None], dt.type(0), b)
    delta = a * b.T.dot(w.T)
  assert delta.dtype == dt and gamma.dtype == dt
  return delta, gamma


def lda_step(x, n, alpha, eta, iters, want_delta=True, want_doc_topics=True):
  """One step on a tile of documents as new tiles (delta [k, V], doc_topics [D, k]; None for one that is not wanted);
  `x` [V, D] and `n` [k, V] both float32 or both float64."""
  if isinstance(x, distarray.Absent) or isinstance(n, distarray.Absent):
    v, d, k, dt = x.shape[0], x.shape[1], n.shape[0], np.dtype(x.dtype)
    return (distarray.Absent((k, v), dt) if want_delta else None,
            distarray.Absent((d, k), dt) if want_doc_topics else None)
  be = context.get().backend
  fn = getattr(be, 'lda_step', None)
  if fn is not None:
    return fn(x, n, alpha, eta, iters, want_delta=want_delta, want_doc_topics=want_doc_topics)
  xh, nh = np.asarray(be.to_numpy(x)), np.asarray(be.to_numpy(n))
  alpha, eta, iters = tile_checks.check_lda_step((xh.dtype, nh.dtype), (xh.shape, nh.shape), alpha, eta, iters)[4:7]
  delta, doc_topics = step_numpy(xh, nh, alpha, eta, iters)
  return (delta if want_delta else None, doc_topics if want_doc_topics else None)
