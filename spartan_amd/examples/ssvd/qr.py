"""Thin QR factorisation of a tall matrix by Cholesky-QR (interface of the reference's spartan/examples/ssvd/qr.py:
`qr(Y)` -> (Q, R), the first step of its ssvd / svd / pca).

  Y^T Y   the K-split dot of the row tiles (one GEMM per tile, partial products added)
  R       = potrf(Y^T Y)^T                 on the device (sp_potrf); returned as a NumPy array
  Q       per row tile, Q_i . R = Y_i      by substitution against L = R^T (sp_trsm_rlt); a distributed array

Deviation from the reference's arithmetic: the reference forms inv(R) with numpy.linalg.inv and multiplies, Q = Y .
inv(R); here Q is the SOLUTION of Q . R = Y.  The two agree to rounding; the solve carries the componentwise backward
error bound of substitution, |Q . R - Y| <= gamma_K |Q| |R|, which a product with a computed inverse does not.
"""
import numpy as np

from ... import context, expr
from ...array import extent
from .. import _dense


def _solve_mapper(extents, tiles, low=None):
  yield extents[0], _dense.trsm_rlt(tiles[0], low)


_solve_mapper.yields_fresh_tensors = True      # kernel outputs (or LAPACK's), never the fetched row tile


def qr(Y):
  """(Q, R) with Q . R = Y: Y an (M, K) expression tiled by rows, K small enough for Y^T Y to fit one tile and Y of full
  column rank.  Q is a distributed (M, K) array, R a NumPy (K, K) upper triangular array with a positive diagonal."""
  be = context.get().backend
  gram = expr.dot(expr.transpose(Y), Y).optimized().evaluate()
  whole = gram.fetch(extent.from_shape(gram.shape))          # one tile (K x K), where the factorisation runs
  low = _dense.potrf(whole)
  R = np.ascontiguousarray(np.asarray(be.to_numpy(low)).T)
  Q = expr.map2(Y, (0,), fn=_solve_mapper, fn_kw={'low': low}, shape=tuple(Y.shape)).evaluate()
  return Q, R
