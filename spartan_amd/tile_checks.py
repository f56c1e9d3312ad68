"""What the tile bodies outside the fused path refuse, one pure function per operation.

check_<op>(dtypes, shapes, parameters ...) returns the normalised values of a call (dtype, sizes, int(k), float(m) ...)
or raises.  It is the one copy: HipBackend.<op> (backend_hip_extras.py), the launcher kernels.<op> and the NumPy body
under examples/ all refuse through it, so that a condition is refused with one class and one text whichever path a tile
takes.  NumPy only -- no ctypes, no backend, no device: `dtypes` and `shapes` are those of the operands in the order of
the call.  Where a launcher also writes targets of the operands' dtype it appends their dtypes to `dtypes`; the shapes
of targets, strides and where the bytes live stay with the launcher, which alone can know them.  The limits (*_MAX_*)
stand in _hip.py beside the ABI table they restate.
"""
import math

import numpy as np

from . import _hip
from ._hip import refuse_not_float

_I64 = np.dtype(np.int64)


def one_float_dtype(what, dtypes):
  """The one dtype of operands that exist in float32 and float64 only: TypeError for another one, then for two.  (A
  launcher passes the operands' dtype and those of its targets.)"""
  dtypes = [np.dtype(d) for d in dtypes]
  for d in dtypes:
    if d not in _hip.FLOATS:
      refuse_not_float(d, what)
  for d in dtypes[1:]:
    if d != dtypes[0]:
      raise TypeError('%s: operands of two dtypes (%s, %s); convert with astype first' % (what, dtypes[0], d))
  return dtypes[0]


def _shapes(shapes):
  return [tuple(s) for s in shapes]


def _square(what, dtype, shape):
  """(dtype, n) of the one square float32 / float64 operand of potrf, syev and apsp."""
  dtype, shape = np.dtype(dtype), tuple(shape)
  if dtype not in _hip.FLOATS:
    refuse_not_float(dtype, what)
  if len(shape) != 2 or shape[0] != shape[1]:
    raise ValueError('%s: expected a square matrix, got shape %s' % (what, shape))
  return dtype, shape[0]


def check_potrf(dtype, shape):
  """(dtype, n) of a Cholesky factorisation, or TypeError for a matrix that is not float32 / float64 and ValueError for
  one that is not square."""
  return _square('potrf', dtype, shape)


def check_syev(dtype, shape, what='syev'):
  """(dtype, n) of a symmetric eigenproblem; refusals as check_potrf's."""
  return _square(what, dtype, shape)


def check_apsp(dtype, shape):
  """(dtype, n) of an all-pairs shortest-path call on a matrix of edge lengths; refusals as check_potrf's."""
  return _square('apsp', dtype, shape)


def check_trsm_rlt(dtypes, shapes):
  """(dtype, m, n) of x . l^T = b on b [m, n] and l [n, n] -- `dtypes` and `shapes` are theirs, in that order -- or
  TypeError for operands that are not float32 / float64 or of two dtypes, ValueError for shapes that do not fit."""
  dt = one_float_dtype('trsm_rlt', dtypes)
  b, l = _shapes(shapes)
  if len(b) != 2 or len(l) != 2 or l[0] != l[1] or b[1] != l[0]:
    raise ValueError('trsm_rlt: shapes %s and %s do not fit' % (b, l))
  return dt, b[0], b[1]


def check_count(label, value, most):
  """int(value), or ValueError if it is outside 1 .. most; `label` names it ('knn: k').  The drivers check their own
  counts with it too."""
  value = int(value)
  if not 1 <= value <= most:
    raise ValueError('%s = %d is outside 1 .. %d' % (label, value, most))
  return value


def check_finite_positive(label, value):
  """float(value), or ValueError if it is not finite and > 0; `label` names it ('lda_step: alpha')."""
  value = float(value)
  if not (value > 0.0 and value != float('inf')):
    raise ValueError('%s = %r must be finite and > 0' % (label, value))
  return value


def check_float_dtype(dtype, what):
  """`dtype` as a NumPy dtype for the driver `what`, which computes in float32 or float64, or TypeError."""
  dtype = np.dtype(dtype)
  if dtype not in _hip.FLOATS:
    raise TypeError('%s: dtype %s is not supported (float32 float64)' % (what, dtype))
  return dtype


def check_knn(dtypes, shapes, k, splits=0):
  """(dtype, nq, np, d, k, splits) of a nearest-neighbour search of queries [nq, d] among points [np, d], or TypeError
  for operands that are not float32 / float64 or of two dtypes, ValueError for shapes that do not fit, a k outside
  1 .. KNN_MAX_K and splits < 0."""
  dt = one_float_dtype('knn', dtypes)
  q, x = _shapes(shapes)
  if len(q) != 2 or len(x) != 2 or q[1] != x[1]:
    raise ValueError('knn: shapes %s and %s do not fit' % (q, x))
  k, splits = check_count('knn: k', k, _hip.KNN_MAX_K), int(splits)
  if splits < 0:
    raise ValueError('knn: splits = %d is negative' % splits)
  return dt, q[0], x[0], q[1], k, splits


def _check_merge(what, dtypes, shapes, k, most):
  """(dtype, rows, candidates, k) of a merge of candidate lists: values [rows, cands] float32 / float64, indices the
  same shape, int64."""
  dt = np.dtype(dtypes[0])
  if dt not in _hip.FLOATS:
    refuse_not_float(dt, what)
  if np.dtype(dtypes[1]) != _I64:
    raise TypeError('%s: candidate indices of dtype %s (int64 expected); convert with astype first'
                    % (what, np.dtype(dtypes[1])))
  val, idx = tuple(shapes[0]), tuple(shapes[1])
  if len(val) != 2 or val != idx:
    raise ValueError('%s: shapes %s and %s do not fit' % (what, val, idx))
  return dt, val[0], val[1], check_count(what + ': k', k, most)


def check_knn_merge(dtypes, shapes, k):
  """(dtype, nq, m, k) of a merge of nearest-neighbour candidates cand_dist2 and cand_idx, both [nq, m], or TypeError
  for distances that are not float32 / float64 or indices that are not int64, ValueError for shapes that do not fit and
  a k outside 1 .. KNN_MAX_K."""
  return _check_merge('knn_merge', dtypes, shapes, k, _hip.KNN_MAX_K)


def check_item_topk_merge(dtypes, shapes, k):
  """(dtype, m, cands, k) of a merge of similarity candidates cand_sim and cand_idx, both [m, cands]; refusals as
  check_knn_merge's, k up to CF_MAX_K."""
  return _check_merge('item_topk_merge', dtypes, shapes, k, _hip.CF_MAX_K)


def check_graph_from_knn(dtypes, shapes):
  """(dtype, n, k) of the neighbour lists dist and idx, both [n, k], or TypeError for weights that are not float32 /
  float64 or indices that are not int64, ValueError for shapes that do not fit."""
  dt = np.dtype(dtypes[0])
  if dt not in _hip.FLOATS:
    refuse_not_float(dt, 'graph_from_knn')
  if np.dtype(dtypes[1]) != _I64:
    raise TypeError('graph_from_knn: indices of dtype %s (int64 expected); convert with astype first'
                    % (np.dtype(dtypes[1]),))
  dist, idx = tuple(shapes[0]), tuple(shapes[1])
  if len(dist) != 2 or dist != idx:
    raise ValueError('graph_from_knn: shapes %s and %s do not fit' % (dist, idx))
  return dt, dist[0], dist[1]


def check_als_solve(dtypes, shapes):
  """(dtype, m, n, f) of an ALS half-step on ratings [m, n] and factors [n, f], or TypeError for operands that are not
  float32 / float64 or of two dtypes, ValueError for shapes that do not fit and an f outside 1 .. SP_ALS_MAX_F."""
  dt = one_float_dtype('als_solve', dtypes)
  r, y = _shapes(shapes)
  if len(r) != 2 or len(y) != 2 or r[1] != y[0]:
    raise ValueError('als_solve: shapes %s and %s do not fit' % (r, y))
  return dt, r[0], r[1], check_count('als_solve: f', y[1], _hip.SP_ALS_MAX_F)


def check_fuzzy_m(m, what='fuzzy_step'):
  """The fuzziness m as a float, or ValueError if it is not finite and > 1."""
  m = float(m)
  if not (m > 1.0 and m != float('inf')):
    raise ValueError('%s: m = %r must be finite and > 1' % (what, m))
  return m


def check_fuzzy_step(dtypes, shapes, m, splits=0):
  """(dtype, n, k, d, m, splits) of a fuzzy k-means step on points [n, d] and centers [k, d], or TypeError for operands
  that are not float32 / float64 or of two dtypes, ValueError for an m that is not finite and > 1, shapes that do not
  fit, k < 1 and splits < 0."""
  dt = one_float_dtype('fuzzy_step', dtypes)
  m = check_fuzzy_m(m)
  x, c = _shapes(shapes)
  if len(x) != 2 or len(c) != 2 or x[1] != c[1]:
    raise ValueError('fuzzy_step: shapes %s and %s do not fit' % (x, c))
  if c[0] < 1:
    raise ValueError('fuzzy_step: k = %d must be at least 1' % c[0])
  splits = int(splits)
  if splits < 0:
    raise ValueError('fuzzy_step: splits = %d' % splits)
  return dt, x[0], c[0], x[1], m, splits


def check_lda_params(k, alpha, eta, iters, what='lda_step'):
  """(k, alpha, eta, iters) as sp_lda_step takes them, or ValueError for a k outside 1 .. SP_LDA_MAX_K, iters < 1 and
  an alpha or eta that is not finite and > 0."""
  k, iters, alpha, eta = int(k), int(iters), float(alpha), float(eta)
  if not 1 <= k <= _hip.SP_LDA_MAX_K:
    raise ValueError('%s: k = %d must be in 1 .. %d' % (what, k, _hip.SP_LDA_MAX_K))
  if iters < 1:
    raise ValueError('%s: iters = %d must be at least 1' % (what, iters))
  return k, check_finite_positive(what + ': alpha', alpha), check_finite_positive(what + ': eta', eta), iters


def check_lda_step(dtypes, shapes, alpha, eta, iters, splits=0):
  """(dtype, V, D, k, alpha, eta, iters, splits) of a CVB0 step on x [V, D] and n [k, V], or TypeError for operands that
  are not float32 / float64 or of two dtypes, ValueError for shapes that do not fit, what check_lda_params refuses and
  splits < 0."""
  dt = one_float_dtype('lda_step', dtypes)
  x, n = _shapes(shapes)
  if len(x) != 2 or len(n) != 2 or x[0] != n[1]:
    raise ValueError('lda_step: shapes %s and %s do not fit' % (x, n))
  k, alpha, eta, iters = check_lda_params(n[0], alpha, eta, iters)
  splits = int(splits)
  if splits < 0:
    raise ValueError('lda_step: splits = %d' % splits)
  return dt, x[0], x[1], k, alpha, eta, iters, splits


def check_affinity_params(metric, gamma, what='affinity'):
  """(the library's code of `metric`, gamma as a float), or what sp_affinity_* refuses: NotImplementedError for
  'scaled_euclidean', ValueError for an unknown metric or a gamma that is not finite.  The one copy: the launchers, the
  backend and the NumPy bodies of examples/_spectral.py all refuse through it."""
  if metric == 'scaled_euclidean':
    raise NotImplementedError("%s: 'scaled_euclidean' is refused: the reference calls np.square(X, Y), which writes X "
                              "squared INTO its second operand, so its result depends on the order in which the pairs "
                              "are visited" % what)
  if metric not in _hip.SP_AFF_METRICS:
    raise ValueError('%s: unknown metric %r (%s)' % (what, metric, ' '.join(sorted(_hip.SP_AFF_METRICS))))
  gamma = float(gamma)
  if not math.isfinite(gamma):
    raise ValueError('%s: gamma = %r must be finite' % (what, gamma))
  return _hip.SP_AFF_METRICS[metric], gamma


def _affinity_operands(what, dtypes, x, y):
  dt = one_float_dtype(what, dtypes)
  x, y = tuple(x), tuple(y)
  if len(x) != 2 or len(y) != 2 or x[1] != y[1]:
    raise ValueError('%s: shapes %s and %s do not fit' % (what, x, y))
  return dt, x[0], y[0], x[1]


def check_affinity_degree(dtypes, shapes, metric, gamma):
  """(dtype, m, n, d, the metric's code, gamma) of the degrees of x [m, d] against y [n, d], or TypeError for operands
  that are not float32 / float64 or of two dtypes, ValueError for shapes that do not fit, then what
  check_affinity_params refuses."""
  dt, m, n, d = _affinity_operands('affinity_degree', dtypes, *shapes)
  return (dt, m, n, d) + check_affinity_params(metric, gamma, 'affinity_degree')


def check_affinity_matrix(dtypes, shapes, r0, metric, gamma):
  """(dtype, m, n, d, the metric's code, gamma, r0) of the affinities of x [m, d], points r0 .. r0 + m - 1 of y [n, d],
  against y -- `dtypes` and `shapes` are those of x, y and, where one is passed, of scale [n] -- or the refusals of
  check_affinity_degree, then ValueError for rows that are not among the points and a scale that is not [n]."""
  dt, m, n, d = _affinity_operands('affinity_matrix', dtypes, shapes[0], shapes[1])
  code, gamma = check_affinity_params(metric, gamma, 'affinity_matrix')
  r0 = int(r0)
  if r0 < 0 or r0 + m > n:
    raise ValueError('affinity_matrix: rows %d .. %d are not among the %d points' % (r0, r0 + m, n))
  if len(shapes) > 2 and tuple(shapes[2]) != (n,):
    raise ValueError('affinity_matrix: a scale of shape %s for %d points' % (tuple(shapes[2]), n))
  return dt, m, n, d, code, gamma, r0


def check_nb_operands(x_dtype, x_shape, labels_dtype, labels_shape, label_size, splits=0, what='nb_step'):
  """(m, d, label_size) of the operands of a naive Bayes step, or what sp_nb_step refuses: TypeError for data that is
  not float32 / float64 or labels that are not int64, ValueError for label_size outside 1 .. 128, data that is not 2-D,
  labels that are not [m] or [m, 1] and splits < 0.  The one copy: the launcher, the backend and the NumPy body of
  examples/_nb.py all refuse through it."""
  if np.dtype(x_dtype) not in _hip.FLOATS:
    raise TypeError('%s: dtype %s is not supported (float32 float64); convert with astype first' % (what, np.dtype(x_dtype)))
  if np.dtype(labels_dtype) != _I64:
    raise TypeError('%s: labels of dtype %s; convert with astype(int64) first' % (what, np.dtype(labels_dtype)))
  label_size = int(label_size)
  if not 1 <= label_size <= _hip.SP_NB_MAX_LABELS:
    raise ValueError('%s: label_size = %d must be in 1 .. %d' % (what, label_size, _hip.SP_NB_MAX_LABELS))
  x_shape, labels_shape = tuple(int(v) for v in x_shape), tuple(int(v) for v in labels_shape)
  if len(x_shape) != 2:
    raise ValueError('%s: expected data of shape (m, d), got %s' % (what, x_shape))
  if labels_shape not in ((x_shape[0],), (x_shape[0], 1)):
    raise ValueError('%s: labels of shape %s for %d rows' % (what, labels_shape, x_shape[0]))
  if int(splits) < 0:
    raise ValueError('%s: splits = %d' % (what, splits))
  return x_shape[0], x_shape[1], label_size


def check_nbody_operands(dtypes, shapes, r0, m, g, rmin, splits=0, what='nbody_accel'):
  """(dtype, n, r0, m, g, rmin, splits) of an all-pairs gravity call on x, y, z and mass -- `dtypes` and `shapes` are
  theirs, in that order -- or what sp_nbody_accel refuses: TypeError ("astype first") for arrays that are not float32 /
  float64 or that are of two dtypes; ValueError for arrays that are not 1-D and of equal length, targets r0 .. r0 + m
  that are not among the n bodies, splits < 0, a g that is not finite in the arrays' dtype and an rmin that is not
  finite and > 0 in it.  The one copy: the launcher, the backend, the NumPy body of examples/_nbody.py and the driver
  all refuse through it."""
  dtypes = [np.dtype(d) for d in dtypes]
  for d in dtypes:
    if d not in _hip.FLOATS:
      raise TypeError('%s: dtype %s is not supported (float32 float64); convert with astype first' % (what, d))
  for d in dtypes[1:]:
    if d != dtypes[0]:
      raise TypeError('%s: operands of two dtypes (%s, %s); convert with astype first' % (what, dtypes[0], d))
  shapes = [tuple(int(v) for v in s) for s in shapes]
  if any(len(s) != 1 for s in shapes) or any(s != shapes[0] for s in shapes):
    raise ValueError('%s: x, y, z and mass must be 1-D and of equal length, got shapes %s' % (what, shapes))
  n, r0, m, splits = shapes[0][0], int(r0), int(m), int(splits)
  if r0 < 0 or m < 0 or r0 + m > n:
    raise ValueError('%s: bodies %d .. %d are not among the %d' % (what, r0, r0 + m, n))
  if splits < 0:
    raise ValueError('%s: splits = %d' % (what, splits))
  g, rmin = float(g), float(rmin)
  with np.errstate(all='ignore'):
    gt, rt = dtypes[0].type(g), dtypes[0].type(rmin)
  if not np.isfinite(gt):
    raise ValueError('%s: g = %r must be finite in %s' % (what, g, dtypes[0]))
  if not (rt > 0 and np.isfinite(rt)):
    raise ValueError('%s: rmin = %r must be finite and > 0 in %s' % (what, rmin, dtypes[0]))
  return dtypes[0], n, r0, m, g, rmin, splits


def check_item_topk_operands(dtypes, t_shape, tnorm_shape, s_shape, snorm_shape, k, splits=0, what='item_topk'):
  """(dtype, users, m, ns, k, splits) of a cosine top-k call on targets [users, m], tnorm [m], sources [users, ns] and
  snorm [ns] -- `dtypes` are theirs, in that order -- or what sp_item_topk refuses: TypeError ("astype first") for
  operands that are not float32 / float64 or that are of two dtypes; ValueError for targets or sources that are not 2-D,
  user counts that differ, norms that are not [m] and [ns], a k outside 1 .. CF_MAX_K and splits < 0.  The one copy:
  the launcher, the backend, the NumPy body of examples/cf/_cf.py and the driver all refuse through it."""
  dtypes = [np.dtype(d) for d in dtypes]
  for d in dtypes:
    if d not in _hip.FLOATS:
      raise TypeError('%s: dtype %s is not supported (float32 float64); convert with astype first' % (what, d))
  for d in dtypes[1:]:
    if d != dtypes[0]:
      raise TypeError('%s: operands of two dtypes (%s, %s); convert with astype first' % (what, dtypes[0], d))
  t_shape, s_shape = tuple(int(v) for v in t_shape), tuple(int(v) for v in s_shape)
  tnorm_shape, snorm_shape = tuple(int(v) for v in tnorm_shape), tuple(int(v) for v in snorm_shape)
  if len(t_shape) != 2 or len(s_shape) != 2:
    raise ValueError('%s: targets and sources must be 2-D [users, items], got shapes %s and %s' % (what, t_shape, s_shape))
  if t_shape[0] != s_shape[0]:
    raise ValueError('%s: targets of %d users against sources of %d' % (what, t_shape[0], s_shape[0]))
  if tnorm_shape != (t_shape[1],) or snorm_shape != (s_shape[1],):
    raise ValueError('%s: norms of shapes %s and %s for %d targets and %d sources'
                     % (what, tnorm_shape, snorm_shape, t_shape[1], s_shape[1]))
  k, splits = int(k), int(splits)
  if not 1 <= k <= _hip.CF_MAX_K:
    raise ValueError('%s: k = %d is outside 1 .. %d' % (what, k, _hip.CF_MAX_K))
  if splits < 0:
    raise ValueError('%s: splits = %d is negative' % (what, splits))
  return dtypes[0], t_shape[0], t_shape[1], s_shape[1], k, splits


def check_svm_dca(dtypes, shapes, scaled_lambda, chains=1, what='svm_dca'):
  """(dtype, m, d, scaled_lambda, chains) of a dual coordinate ascent pass on x [m, d], y, alpha and w0 -- `dtypes` and
  `shapes` are theirs, in that order -- or what sp_svm_dca refuses: TypeError ("astype first") for arrays that are not
  float32 / float64 or that are of two dtypes; ValueError for an x that is not 2-D, a y or alpha that is not [m] or
  [m, 1], a w0 that is not [d] or [d, 1], a d outside 1 .. SP_SVM_MAX_D, chains < 1 and a scaled_lambda that is not
  finite and > 0 in the arrays' dtype.  The one copy: the launcher, the backend, the NumPy body of examples/_svm.py and
  the driver all refuse through it."""
  dtypes = [np.dtype(d) for d in dtypes]
  for d in dtypes:
    if d not in _hip.FLOATS:
      raise TypeError('%s: dtype %s is not supported (float32 float64); convert with astype first' % (what, d))
  for d in dtypes[1:]:
    if d != dtypes[0]:
      raise TypeError('%s: operands of two dtypes (%s, %s); convert with astype first' % (what, dtypes[0], d))
  x, y, alpha, w0 = (tuple(int(v) for v in s) for s in shapes)
  if len(x) != 2:
    raise ValueError('%s: expected data of shape (m, d), got %s' % (what, x))
  m, d = x
  for name, shape in (('y', y), ('alpha', alpha)):
    if shape not in ((m,), (m, 1)):
      raise ValueError('%s: %s of shape %s for %d rows' % (what, name, shape, m))
  if not 1 <= d <= _hip.SP_SVM_MAX_D:
    raise ValueError('%s: d = %d must be in 1 .. %d' % (what, d, _hip.SP_SVM_MAX_D))
  if w0 not in ((d,), (d, 1)):
    raise ValueError('%s: w0 of shape %s for %d features' % (what, w0, d))
  chains = int(chains)
  if chains < 1:
    raise ValueError('%s: chains = %d must be at least 1' % (what, chains))
  scaled_lambda = float(scaled_lambda)
  with np.errstate(all='ignore'):
    st = dtypes[0].type(scaled_lambda)
  if not (st > 0 and np.isfinite(st)):
    raise ValueError('%s: scaled_lambda = %r must be finite and > 0 in %s' % (what, scaled_lambda, dtypes[0]))
  return dtypes[0], m, d, scaled_lambda, chains


def check_sgd_mf(dtypes, tile_shape, u_shape, m_shape, lr=None, what='sgd_mf'):
  """(dtype, m, n, f, lr) of one SGD pass over a tile of ratings [m, n] with the factors U [m, f] and M [n, f] --
  `dtypes` are those of the tile's values, of U and of M -- or what sp_sgd_mf refuses: TypeError ("astype first") for
  arrays that are not float32 / float64 or that are of two dtypes; ValueError for a tile that is not 2-D, a U that is
  not [m, f], an M that is not [n, f], an f outside 1 .. SP_MF_MAX_F and an lr that is not finite in the arrays' dtype.
  lr = None is the reference's float32(1e-5).  The one copy: the launcher, the backend, the NumPy body of
  examples/_netflix.py and the driver all refuse through it."""
  dtypes = [np.dtype(d) for d in dtypes]
  for d in dtypes:
    if d not in _hip.FLOATS:
      raise TypeError('%s: dtype %s is not supported (float32 float64); convert with astype first' % (what, d))
  for d in dtypes[1:]:
    if d != dtypes[0]:
      raise TypeError('%s: operands of two dtypes (%s, %s); convert with astype first' % (what, dtypes[0], d))
  v, u, mm = (tuple(int(s) for s in shape) for shape in (tile_shape, u_shape, m_shape))
  if len(v) != 2:
    raise ValueError('%s: expected ratings of shape (m, n), got %s' % (what, v))
  m, n = v
  if len(u) != 2 or u[0] != m:
    raise ValueError('%s: U of shape %s for %d rows of ratings' % (what, u, m))
  f = u[1]
  if not 1 <= f <= _hip.SP_MF_MAX_F:
    raise ValueError('%s: rank f = %d must be in 1 .. %d' % (what, f, _hip.SP_MF_MAX_F))
  if mm != (n, f):
    raise ValueError('%s: M of shape %s for %d columns of ratings and rank %d' % (what, mm, n, f))
  lr = float(np.float32(1e-5)) if lr is None else float(lr)
  with np.errstate(all='ignore'):
    lt = dtypes[0].type(lr)
  if not np.isfinite(lt):
    raise ValueError('%s: lr = %r must be finite in %s' % (what, lr, dtypes[0]))
  return dtypes[0], m, n, f, lr


def check_lmm_swaption(dtype, shape, maturities, lamb, delta, f0, theta, steps=None, what='lmm_swaption'):
  """(dtype, n, S, K, lamb, delta, f0, theta) of one swaption's paths from draws eps [S, n] -- `dtype` and `shape` are
  theirs -- over K = `maturities` forward rates, or what sp_lmm_swaption refuses: TypeError ("astype first") for draws
  that are not float32 / float64; ValueError for draws that are not 2-D (with `steps` rows, where the caller names
  them), S and K that do not satisfy 1 <= S < K <= SP_LMM_MAX_K, a lamb, delta, f0 or theta that is not finite in the
  draws' dtype, and delta <= 0.  The one copy: the launcher, the backend, the NumPy body of examples/_swaption.py and
  the driver all refuse through it."""
  dtype = np.dtype(dtype)
  if dtype not in _hip.FLOATS:
    raise TypeError('%s: dtype %s is not supported (float32 float64); convert with astype first' % (what, dtype))
  shape = tuple(int(v) for v in shape)
  if len(shape) != 2 or (steps is not None and shape[0] != int(steps)):
    raise ValueError('%s: expected draws of shape (%s, n), got %s' % (what, 'steps' if steps is None else int(steps), shape))
  s, n = shape
  k = int(maturities)
  if not 1 <= s < k <= _hip.SP_LMM_MAX_K:
    raise ValueError('%s: steps = %d and maturities = %d must satisfy 1 <= steps < maturities <= %d'
                     % (what, s, k, _hip.SP_LMM_MAX_K))
  scalars = []
  for name, value in (('lamb', lamb), ('delta', delta), ('f0', f0), ('theta', theta)):
    value = float(value)
    with np.errstate(all='ignore'):
      vt = dtype.type(value)
    if not np.isfinite(vt):
      raise ValueError('%s: %s = %r must be finite in %s' % (what, name, value, dtype))
    if name == 'delta' and not vt > 0:
      raise ValueError('%s: delta = %r must be > 0 in %s' % (what, value, dtype))
    scalars.append(value)
  return (dtype, n, s, k) + tuple(scalars)


def _canopy_floats(what, dtypes):
  dtypes = [np.dtype(d) for d in dtypes]
  for d in dtypes:
    if d not in _hip.FLOATS:
      raise TypeError('%s: dtype %s is not supported (float32 float64); convert with astype first' % (what, d))
  for d in dtypes[1:]:
    if d != dtypes[0]:
      raise TypeError('%s: operands of two dtypes (%s, %s); convert with astype first' % (what, dtypes[0], d))
  return dtypes[0]


_NO_CF = object()


def check_canopy(dtype, shape, t1, t2, chains=1, cap=None, cf=_NO_CF, what='canopy'):
  """(dtype, n, d, t1, t2, chains, cap, cf) of the greedy canopy pass over points x [n, d] -- `dtype` and `shape` are
  theirs -- or what sp_canopy refuses: TypeError ("astype first") for points that are not float32 / float64; ValueError
  for points that are not 2-D, d < 1, chains < 1, cap < 1, and a t1 or t2 that is not finite in the points' dtype.
  cap = None is min(the longest chain's rows, 1024), at least 1.  `cf`, the caller's filter `count > cf`, is returned as
  an int (None where the caller gives none): ValueError for one that is not an integer.  The one copy: the launcher, the backend, the
  NumPy body of examples/_canopy.py and the driver all refuse through it."""
  dtype = _canopy_floats(what, [dtype])
  shape = tuple(int(v) for v in shape)
  if len(shape) != 2:
    raise ValueError('%s: expected points of shape (n, d), got %s' % (what, shape))
  n, d = shape
  if d < 1:
    raise ValueError('%s: d = %d must be at least 1' % (what, d))
  chains = int(chains)
  if chains < 1:
    raise ValueError('%s: chains = %d must be at least 1' % (what, chains))
  if cap is None:
    cap = max(min(-(-n // chains), 1024), 1)
  cap = int(cap)
  if cap < 1:
    raise ValueError('%s: cap = %d must be at least 1' % (what, cap))
  scalars = []
  for name, value in (('t1', t1), ('t2', t2)):
    value = float(value)
    with np.errstate(all='ignore'):
      vt = dtype.type(value)
    if not np.isfinite(vt):
      raise ValueError('%s: %s = %r must be finite in %s' % (what, name, value, dtype))
    scalars.append(value)
  if cf is _NO_CF:
    cf = None
  else:
    if isinstance(cf, (bool, np.bool_)) or not isinstance(cf, (int, np.integer)):
      raise ValueError('%s: cf = %r must be an integer' % (what, cf))
    cf = int(cf)
  return dtype, n, d, scalars[0], scalars[1], chains, cap, cf


def check_pdf_label(dtypes, shapes, what='pdf_label'):
  """(dtype, n, k, d) of the labels of points x [n, d] among centres [k, d] -- `dtypes` and `shapes` are theirs, in
  that order -- or what sp_pdf_label refuses: TypeError ("astype first") for arrays that are not float32 / float64 or
  that are of two dtypes; ValueError for points or centres that are not 2-D, feature counts that differ and d < 1.
  k = 0 is accepted (every label is -1).  The one copy, as check_canopy."""
  dtype = _canopy_floats(what, dtypes)
  x, c = (tuple(int(v) for v in s) for s in shapes)
  if len(x) != 2:
    raise ValueError('%s: expected points of shape (n, d), got %s' % (what, x))
  if len(c) != 2:
    raise ValueError('%s: expected centers of shape (k, d), got %s' % (what, c))
  if x[1] != c[1]:
    raise ValueError('%s: points of %d features and centers of %d' % (what, x[1], c[1]))
  if x[1] < 1:
    raise ValueError('%s: d = %d must be at least 1' % (what, x[1]))
  return dtype, x[0], c[0], x[1]
