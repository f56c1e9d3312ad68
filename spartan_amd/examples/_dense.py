"""The dense tile bodies the Cholesky, QR and SVD drivers share: backend.potrf / backend.trsm_rlt / backend.syev where
the backend has them (HipBackend: sp_potrf / sp_trsm_rlt / sp_syevj), LAPACK on host arrays otherwise, as in the
reference -- which keeps the drivers runnable on a backend of plain NumPy tiles."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray


def _lapack(name, *arrays):
  from scipy.linalg import lapack
  return lapack.get_lapack_funcs((name,), arrays)[0]


def potrf(t):
  """The lower Cholesky factor of the tile `t` (its lower triangle is read), zero above the diagonal."""
  if isinstance(t, distarray.Absent):
    return t
  be = context.get().backend
  fn = getattr(be, 'potrf', None)
  if fn is not None:
    return fn(t)
  t = np.asarray(be.to_numpy(t))
  tile_checks.check_potrf(t.dtype, t.shape)
  if t.shape[0] == 0:
    return t.copy()
  low, info = _lapack('potrf', t)(t, lower=1, clean=1)
  if info:
    raise np.linalg.LinAlgError('%d-th leading minor of the array is not positive definite' % info)
  return np.ascontiguousarray(low)


def trsm_rlt(b, low):
  """x with x . low^T = b for the lower triangular tile `low`."""
  if isinstance(b, distarray.Absent):
    return b
  be = context.get().backend
  fn = getattr(be, 'trsm_rlt', None)
  if fn is not None:
    return fn(b, low)
  b, low = np.asarray(be.to_numpy(b)), np.asarray(be.to_numpy(low))
  tile_checks.check_trsm_rlt((b.dtype, low.dtype), (b.shape, low.shape))
  if b.size == 0:
    return b.copy()
  xt, info = _lapack('trtrs', low, b)(low, b.T, lower=1)
  if info:
    raise np.linalg.LinAlgError('trsm_rlt: the triangular matrix is singular (zero at position %d of its diagonal)' % info)
  return np.ascontiguousarray(xt.T)


def syev(t):
  """(w, V): the eigenvalues of the symmetric tile `t` (its lower triangle is read) in ascending order and the
  eigenvectors as the columns of V."""
  be = context.get().backend
  fn = getattr(be, 'syev', None)
  if fn is not None:
    return fn(t)
  t = np.asarray(be.to_numpy(t))
  tile_checks.check_syev(t.dtype, t.shape)
  if t.shape[0] == 0:
    return np.empty((0,), t.dtype), t.copy()
  w, v, info = _lapack('syevd', t)(t, lower=1)
  if info:
    raise np.linalg.LinAlgError('Eigenvalues did not converge')
  return w, np.ascontiguousarray(v)
