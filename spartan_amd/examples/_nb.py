"""The tile body of the naive Bayes driver: backend.nb_step where the backend has it (HipBackend: sp_nb_step), NumPy on
host arrays otherwise -- the same formulas, special values and `bad` in the tile's dtype (include/spartan_hip_nb.h),
which keeps the driver runnable on a backend of plain NumPy tiles.  Both paths refuse through one function,
tile_checks.check_nb_operands (the launcher and HipBackend.nb_step call it too)."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray

check_operands = tile_checks.check_nb_operands


def step_numpy(x, labels, label_size):
  """(S [label_size, d] in x's dtype, df int64 [d], bad int64 [1]) of a row tile x [m, d] with int64 labels [m]:
  r_i = sqrt(sum_j x_ij^2 / d), S_l. = the rows x_i. / r_i of label l added onto zeros in row order, df_j = the rows
  with x_ij > 0, bad = 0 or 1 + the lowest row whose label is outside 0 .. label_size - 1 (left out of S, kept in df).
  The sum of squares is NumPy's, in another order than the kernel's; everything else is the kernel's arithmetic."""
  dt = x.dtype
  m, d = x.shape
  labels = labels.reshape(m)
  with np.errstate(all='ignore'):
    q = (x * x).sum(axis=1, dtype=dt)
    r = np.sqrt(q / dt.type(d))
    z = x / r[:, None]
  ok = (labels >= 0) & (labels < label_size)
  s = np.zeros((label_size, d), dt)
  with np.errstate(all='ignore'):
    np.add.at(s, labels[ok], z[ok])              # unbuffered: one row after the other, in row order
  df = (x > 0).sum(axis=0, dtype=np.int64).reshape(d)
  wrong = np.flatnonzero(~ok)
  bad = np.array([wrong[0] + 1 if wrong.size else 0], np.int64)
  assert s.dtype == dt and z.dtype == dt
  return s, df, bad


def nb_step(x, labels, label_size, splits=0):
  """The naive Bayes step of a row tile as new tiles (S [label_size, d], df int64 [d], bad int64 [1]); `x` [m, d]
  float32 or float64, `labels` int64 [m] or [m, 1].  TypeError ("astype first") for other dtypes, ValueError for
  label_size outside 1 .. 128 or shapes that do not fit."""
  if isinstance(x, distarray.Absent) or isinstance(labels, distarray.Absent):
    _, d, label_size = check_operands(x.dtype, x.shape, labels.dtype, labels.shape, label_size)
    return (distarray.Absent((label_size, d), np.dtype(x.dtype)), distarray.Absent((d,), np.dtype(np.int64)),
            distarray.Absent((1,), np.dtype(np.int64)))
  be = context.get().backend
  fn = getattr(be, 'nb_step', None)
  if fn is not None:
    return fn(x, labels, label_size, splits=splits)
  xn, ln = np.asarray(be.to_numpy(x)), np.asarray(be.to_numpy(labels))
  _, _, label_size = check_operands(xn.dtype, xn.shape, ln.dtype, ln.shape, label_size, splits)
  return step_numpy(xn, ln, label_size)
