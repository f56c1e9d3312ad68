"""Alternating least squares (interface of the reference's spartan/examples/als.py: `als(A, la, alpha,
implicit_feedback, num_features, num_iter)` -> (U, M) with A ~ U . M^T, as expressions).

The structure is the reference's: AT = transpose(A); M starts as rand(num_items, num_features) with column 0 set to
the items' average rating, sum(A, 0) * 1.0 / count_nonzero(A, 0); every iteration is two half-steps,
  U = outer((A, M), (0, None), fn=_solve_mapper)        M = outer((AT, U), (0, None), fn=_solve_mapper)
in which a tile body gets a whole row band of ratings and the whole factor matrix and solves every row's normal
equations.  The reference's body is a Python loop over rows around scipy.linalg.lstsq; here it is one call of
_als.als_solve per band (HipBackend: sp_als_solve -- Gram accumulation, Cholesky and substitution fused, nothing of
size m x n x f is written).  Integer ratings are converted to `dtype` on the device.

  explicit   A_i = sum_{r_ij != 0} y_j y_j^T + la |S_i| I,  b_i = sum r_ij y_j;  a row without ratings is exactly 0
  implicit   A_i = Y^T Y + sum_j alpha r_ij y_j y_j^T + la I,  b_i = sum_{r_ij > 0} (1 + alpha r_ij) y_j

Deviations from the reference:
  * an `M` that is passed is used as the starting factors (the reference overwrites its argument with rand): that is
    what makes a run repeatable;
  * `dtype` may be float32 (the reference computes in float64 only);
  * la <= 0 raises ValueError.  The reference's lstsq returns a minimum-norm answer for a singular system; this is a
    Cholesky solve, and with la > 0 every system of explicit mode, and of implicit mode with non-negative ratings, is
    positive definite;
  * num_features > 64 raises ValueError (the kernel keeps a row's whole system in LDS);
  * a system that is not positive definite all the same (negative or NaN ratings, NaN factors -- an item nobody rated
    makes the default M's column 0 NaN, as in the reference) raises numpy.linalg.LinAlgError when U or M is forced:
    one int32 word per als() call is shared by all its solves and read once per forced result.
"""
import numpy as np

from .. import _hip, context, expr, tile_checks
from ..array import distarray, extent
from ..expr import base
from . import _als


def _solve_mapper(ex_a, ratings, ex_b, factors, la=None, alpha=None, implicit=None, shape=None, dtype=None, info=None):
  """Tile body: the rows of U (or M) under this row band of ratings."""
  be = context.get().backend
  if not isinstance(ratings, distarray.Absent):
    ratings = be.astype(ratings, dtype)
  if not isinstance(factors, distarray.Absent):
    factors = be.astype(factors, dtype)
  target = extent.create((ex_a.ul[0], 0), (ex_a.lr[0], shape[1]), shape)
  yield target, _als.als_solve(ratings, factors, la, alpha, implicit, info=info)


_solve_mapper.yields_fresh_tensors = True      # the kernel's output (or NumPy's), never a fetched tile


class _CheckedExpr(base.Expr):
  """`array`, and numpy.linalg.LinAlgError when it is forced if the solves that share `info` flagged a row."""
  members = ('array', 'info')

  def dependencies(self):
    return {'array': self.array}

  def visit(self, visitor):
    return base.expr_like(self, array=visitor.visit(self.array), info=self.info)

  def compute_shape(self):
    return self.array.shape

  def _evaluate(self, ctx, deps):
    flagged = int(np.asarray(ctx.backend.to_numpy(self.info)).reshape(-1)[0])     # the one wait for the device
    if flagged:
      raise np.linalg.LinAlgError('als: the normal equations of row %d of a half-step are not positive definite '
                                  '(negative or NaN ratings, or NaN factors)' % (flagged - 1))
    return deps['array']


def als(A, la=0.065, alpha=40, implicit_feedback=False, num_features=20, num_iter=10, M=None, dtype=np.float64):
  """(U, M), expressions of shape (num_users, num_features) and (num_items, num_features) in `dtype` (float64 or
  float32), after num_iter iterations on the rating matrix `A` (expression / distributed array / NumPy array; 0 = not
  rated).  la: the regulariser; alpha: the confidence weight of implicit feedback; M: the starting item factors
  (default: the reference's rand with the average rating in column 0).  See the module docstring for the deviations."""
  dtype = tile_checks.check_float_dtype(dtype, 'als')
  if not la > 0:
    raise ValueError('als: la = %r must be positive (the solve is a Cholesky factorisation)' % (la,))
  num_features = tile_checks.check_count('als: num_features', num_features, _hip.SP_ALS_MAX_F)
  if num_iter < 1:
    raise ValueError('als: num_iter = %d' % num_iter)
  if isinstance(A, np.ndarray):
    A = expr.from_numpy(A)
  if len(A.shape) != 2:
    raise ValueError('als: expected a rating matrix, got shape %s' % (tuple(A.shape),))
  num_users, num_items = (int(v) for v in A.shape)
  AT = expr.transpose(A)
  if M is None:
    avg_rating = expr.sum(A, axis=0) * 1.0 / expr.count_nonzero(A, axis=0)
    M = expr.rand(num_items, num_features)
    M = expr.assign(M, np.s_[:, 0], expr.reshape(avg_rating, (num_items, 1)))
  else:
    if isinstance(M, np.ndarray):
      M = expr.from_numpy(M)
    if tuple(M.shape) != (num_items, num_features):
      raise ValueError('als: M of shape %s for %d items and %d features' % (tuple(M.shape), num_items, num_features))
  info = context.get().backend.zeros((1,), np.int32)
  kw = {'la': float(la), 'alpha': float(alpha), 'implicit': bool(implicit_feedback), 'dtype': dtype, 'info': info}
  for _ in range(num_iter):
    shape = (num_users, num_features)
    U = expr.outer((A, M), (0, None), fn=_solve_mapper, fn_kw=dict(kw, shape=shape), shape=shape, dtype=dtype)
    shape = (num_items, num_features)
    M = expr.outer((AT, U), (0, None), fn=_solve_mapper, fn_kw=dict(kw, shape=shape), shape=shape, dtype=dtype)
  return _CheckedExpr(array=U, info=info), _CheckedExpr(array=M, info=info)
