"""Stochastic SVD of a tall matrix (interface of the reference's spartan/examples/ssvd/ssvd.py: `svd(A, k)` ->
(U, S, V^T)), every step on device tiles:

  Y      = A . Omega            Omega an (N, k) standard normal draw (expr.randn), or the caller's `omega`
  Q, R   = qr(Y)                the thin Cholesky-QR of examples/ssvd/qr.py (sp_potrf, sp_trsm_rlt)
  B      = Q^T . A              (k, N), one tile
  w, U_  = syev(B . B^T)        the k x k symmetric eigenproblem on ONE tile (sp_syevj on the HIP backend)
  S      = sqrt(max(w, 0))      sorted from large to small, U_'s columns with it
  U      = Q . U_               a distributed (M, k) array, tiled by rows as Y and Q are
  V^T    = (B^T . U_ . diag(1 / S))^T

Deviation from the reference's arithmetic: the reference calls numpy.linalg.eig on a host copy of B . B^T.  On a
matrix that is symmetric only to rounding, eig (the unsymmetric solver) may return complex pairs and returns the
eigenvalues in no order; here a symmetric solver reads the lower triangle, so the eigenvalues are real and ordered,
and the ones rounding has pushed below zero (rank of A below k) are clamped at 0 before the square root.  S and V^T
are returned as NumPy arrays, as in the reference; a zero singular value leaves its row of V^T non-finite, as there.
`omega` is an extension (the tests fix the draw with it); the internal draw is cast to A's dtype, where the
reference's float64 draw would promote a float32 product.
"""
import numpy as np

from ... import context, expr
from ...array import extent
from ...expr.base import Expr
from .. import _dense
from .qr import qr


def svd(A, k=None, omega=None):
  """(U, S, VT) with A ~ U . diag(S) . VT: A an (M, N) array or expression tiled by rows, M >= N; k (default N) the
  number of singular values and vectors.  U is a distributed (M, k) array; S, of shape (k,) and descending, and VT, of
  shape (k, N), are NumPy arrays.  A . Omega must have full column rank k (see qr)."""
  be = context.get().backend
  if isinstance(A, Expr):
    A = A.evaluate()
  if len(A.shape) != 2:
    raise ValueError('svd: expected a matrix, got shape %s' % (tuple(A.shape),))
  n = int(A.shape[1])
  k = n if k is None else int(k)
  if omega is None:
    omega = expr.astype(expr.randn(n, k), A.dtype).evaluate()
  if tuple(omega.shape) != (n, k):
    raise ValueError('svd: omega of shape %s, expected %s' % (tuple(omega.shape), (n, k)))
  rows = int(A.tile_shape()[0])
  Y = expr.dot(A, omega, tile_hint=(rows, k)).optimized().evaluate()
  Q, R = qr(Y)
  B = expr.dot(expr.transpose(Q), A).optimized().evaluate()           # (k, N), one tile
  gram = expr.dot(B, expr.transpose(B)).optimized().evaluate()
  w, vecs = _dense.syev(gram.fetch(extent.from_shape(gram.shape)))    # ascending, on the tile's device
  w, vecs = np.asarray(be.to_numpy(w)), np.asarray(be.to_numpy(vecs))
  S = np.sqrt(np.maximum(w, 0))[::-1].copy()
  U_ = np.ascontiguousarray(vecs[:, ::-1])
  U = expr.dot(Q, U_).optimized().evaluate()
  b_host = np.asarray(be.to_numpy(B.fetch(extent.from_shape(B.shape))))
  with np.errstate(divide='ignore', invalid='ignore'):
    V = b_host.T.dot(U_) * (np.ones(k, S.dtype) / S)
  return U, S, np.ascontiguousarray(V.T)
