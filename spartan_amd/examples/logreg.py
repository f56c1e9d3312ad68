"""Logistic-regression fit by full-batch gradient steps: the other member of the reference's SGD family
(reference: spartan/examples/logistic_regression.py:6-26 on the base class spartan/examples/sgd.py:6-39, which
linear_regression.py shares -- examples/lreg.py here).

One step, for X (N, D) row-tiled over the workers, y (N, 1) and driver-side weights w (D, 1), as
logistic_regression.py:15-17 and sgd.py:36-38 state it:

    g    = exp(X . w)          dot with a driver array, then an element-wise map over its (N, 1) result
    yp   = g / (g + 1)         (the reference's spelling of the sigmoid: NaN where exp overflows, and kept so)
    grad = sum(X * (yp - y), axis=0)
    w   -= alpha * grad        every rank holds the same w -- as the backend's tensor between steps (lreg._whole)

so X is streamed twice per step as stated; on the HIP backend the optimizer rewrites the gradient's DAG into ONE
pass over X (expr/rowdot.py with the exp-ratio link: sp_rowdot_link_colsum_f32 -- the exp and the divide are per ROW,
the rows stay in registers between their two uses).  The same sums in another order; FLAGS['opt_rowdot_fusion'] =
False keeps the launches the expression states.
"""
import numpy as np

from .. import context, expr
from .lreg import _whole, initial_weights


def gradient(x, y, w):
  """Expr of shape (D,): sum over the rows of x * (yp - y), yp = exp(x.w) / (exp(x.w) + 1)."""
  g = expr.exp(expr.dot(x, w))
  yp = g / (g + 1)
  return expr.sum(x * (yp - y), axis=0)


def fit(x, y, steps, alpha=1e-6, w=None):
  """`steps` gradient steps from `w` (drawn by lreg.initial_weights when None: rank 0 draws, the others receive it);
  returns w, shape (D, 1)."""
  n_features = x.shape[1]
  if w is None:
    w = initial_weights(n_features)
  be = context.get().backend if context.initialized() else None
  for _ in range(steps):
    g = _whole(gradient(x, y, w).optimized().evaluate())
    w = w - g.reshape((n_features, 1)) * alpha
  if not isinstance(w, np.ndarray):
    w = be.to_numpy(w)
  return w


def run(n_rows, n_features, steps):
  """logistic_regression.py:23-26's shape of program: uniform random x and y generated on the workers."""
  return fit(expr.rand(n_rows, n_features), expr.rand(n_rows, 1), steps)
