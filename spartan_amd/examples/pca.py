"""Principal component analysis on the stochastic SVD (interface of the reference's spartan/examples/pca.py:
`PCA(n_components).fit(X, rank)`, `.transform(X)`, `.inverse_transform(X)`), every step on device tiles: the column
means, the centring, svd() of examples/ssvd/ssvd.py and the projections."""
import numpy as np

from .. import expr
from ..array import distarray
from ..expr.base import Expr
from .ssvd.ssvd import svd


class PCA(object):
  """components_ (n_components, n_features), a NumPy array: the leading right singular vectors of the centred data;
  mean_ (n_features,), an expression."""

  def __init__(self, n_components=None):
    self.n_components = n_components

  def fit(self, X, rank=None, omega=None):
    """Fit to the (n_samples, n_features) array X, n_samples >= n_features, of rank `rank` (default: n_features; the
    centred data must have that rank, see svd).  X is not modified: the centred data is a new array.  Returns self.
    `omega` is handed on to svd()."""
    self.mean_ = expr.mean(X, axis=0)
    X = X - self.mean_
    if rank is None:
      rank = min(X.shape[0], X.shape[1])
    _, _, vt = svd(X, rank, omega=omega)
    self.components_ = vt[:self.n_components, :]
    return self

  def transform(self, X):
    """X projected on the components: a NumPy (n_samples, n_components) array."""
    return expr.dot(X - self.mean_, np.ascontiguousarray(self.components_.T)).optimized().glom()

  def inverse_transform(self, X):
    """Back to the original space: a distributed (n_samples, n_features) array for a distributed X, a NumPy array for
    a NumPy X."""
    if isinstance(X, (Expr, distarray.DistArray)):
      return (expr.dot(X, self.components_) + self.mean_).optimized().evaluate()
    return np.dot(X, self.components_) + self.mean_.glom()
