"""Linear SVM by distributed dual coordinate ascent, DisDCA (interface of the reference's
spartan/examples/disdca_svm.py: `fit(data, labels, T, la)` -> the lazy weight vector w (d, 1), `predict(w, new_data)`
-> +1 or -1 for one row; its tests/test_svm.py is the benchmark).

fit, with data (n, d) and labels (n, 1) of +1 / -1 (disdca_svm.py:49-69), starts from w = 0 and alpha = 0 and repeats T
times:

    every row band, from its own copy of w, walks its rows in order (disdca_svm.py:5-25, _svm_disdca_train):
        g  = (y_i - x_i . w) / (s x_i . x_i)         dl = y_i max(0, min(1, y_i (g + a_i))) - a_i
        w  = w + (x_i s) dl                           a_i = a_i + dl            s = bands / (la n)
    w = sum(data * alpha * 1.0 / la / n, axis=0)     (the bands' own w are dropped)

The reference runs the band's loop one interpreted row at a time.  Here ONE shuffle over the row bands of
retile(data, (divup(n, workers), d)) -- the reference's calc_tile_hint(data, axis=0) -- calls _svm.svm_dca on each
(HipBackend: sp_svm_dca, the whole loop in one kernel with w on chip) into the (n, 1) alpha target, and the
reference's own expression for w runs on the map and reduce kernels.  include/spartan_hip_svm.h states the order of
the two inner products of a row; everything else is the reference's arithmetic, operation for operation.

Additions: `dtype` (float32 data runs in float32; integer data is converted to float64; `dtype` forces either);
`chains_per_tile` = c cuts every band into c consecutive chains, each from its own copy of w, with s = bands c / (la n)
-- mathematically the reference run on c times as many tiles; `fit_state` returns (w, alpha), both evaluated;
`predict_labels(w, data)` is an expression of +1 / -1 per row, (n, 1) int64.  Labels of shape (n,) or (n, 1) and of
any real dtype are converted with astype.  Deviations: la not finite or <= 0, T < 0, chains_per_tile < 1, data that is
not 2-D, d outside 1 .. 4096 and labels that are not of n rows raise ValueError; complex or object arrays raise
TypeError."""
import numpy as np

from .. import _hip, context, expr, tile_checks, util
from ..array import extent
from . import _svm

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _dca_mapper(array, ex, labels=None, alpha=None, w=None, scaled_lambda=None, chains=None):
  """Tile body of an iteration: the pass over this row band from `w` (a host array), as the band's rows of alpha."""
  if ex.ul[1] != 0:                     # (a band cut by columns as well: its first tile speaks for all of them)
    return []
  lo, hi = ex.ul[0], ex.lr[0]
  x = array.fetch(extent.create((lo, 0), (hi, array.shape[1]), array.shape))
  y = labels.fetch(extent.create((lo, 0), (hi, 1), labels.shape))
  a = alpha.fetch(extent.create((lo, 0), (hi, 1), alpha.shape))
  return [(extent.create((lo, 0), (hi, 1), alpha.shape), _svm.svm_dca(x, y, a, w, scaled_lambda, chains=chains))]


_dca_mapper.yields_fresh_tensors = True      # the kernel's output (or NumPy's), never a fetched tile


def _real(what, a):
  if np.dtype(a.dtype).kind not in 'fiub':
    raise TypeError('fit: %s of dtype %s; the arrays are real numbers' % (what, np.dtype(a.dtype)))


def fit_state(data, labels, T=50, la=1.0, dtype=None, chains_per_tile=1):
  """(w (d, 1), alpha (n, 1)) after T iterations, both evaluated distributed arrays in `dtype`: see `fit`."""
  la = tile_checks.check_finite_positive('fit: la', la)
  T, chains = int(T), int(chains_per_tile)
  if T < 0:
    raise ValueError('fit: T = %d is negative' % T)
  if chains < 1:
    raise ValueError('fit: chains_per_tile = %d must be at least 1' % chains)
  if isinstance(data, np.ndarray):
    _real('data', data)
    data = expr.from_numpy(data)
  if isinstance(labels, np.ndarray):
    _real('labels', labels)
    labels = expr.from_numpy(labels)
  if len(data.shape) != 2:
    raise ValueError('fit: expected data of shape (n, d), got %s' % (tuple(data.shape),))
  n, d = (int(v) for v in data.shape)
  if not 1 <= d <= _hip.SP_SVM_MAX_D:
    raise ValueError('fit: d = %d must be in 1 .. %d' % (d, _hip.SP_SVM_MAX_D))
  if tuple(int(v) for v in labels.shape) not in ((n,), (n, 1)):
    raise ValueError('fit: labels of shape %s for %d rows' % (tuple(labels.shape), n))
  data, labels = expr.evaluate(data), expr.evaluate(labels)
  _real('data', data)
  _real('labels', labels)
  if dtype is None:
    dtype = np.dtype(data.dtype) if np.dtype(data.dtype) in _FLOATS else np.dtype(np.float64)
  dtype = tile_checks.check_float_dtype(dtype, 'fit')
  if np.dtype(data.dtype) != dtype:
    data = expr.evaluate(expr.astype(data, dtype))
  if np.dtype(labels.dtype) != dtype:
    labels = expr.evaluate(expr.astype(labels, dtype))
  if len(labels.shape) == 1:
    labels = expr.evaluate(expr.reshape(labels, (n, 1)))

  band = max(util.divup(n, context.get().num_workers), 1)
  data = expr.evaluate(expr.retile(data, tile_hint=(band, d)))
  tiles = max(len(set(ex.ul[0] for ex in data.tiles if ex.ul[1] == 0)), 1)
  scaled_lambda = tiles * chains * 1.0 / (la * n) if n else 1.0
  one, la_t, n_t = dtype.type(1.0), dtype.type(la), dtype.type(n)      # (Python scalars would promote float32)

  w = expr.evaluate(expr.zeros((d, 1), dtype=dtype, tile_hint=(d, 1)))
  alpha = expr.evaluate(expr.zeros((n, 1), dtype=dtype, tile_hint=(band, 1)))
  for _ in range(T):
    w_host = np.ascontiguousarray(np.asarray(w.glom()), dtype=dtype).reshape(d, 1)
    target = expr.ndarray((n, 1), dtype=dtype, tile_hint=(band, 1))
    alpha = expr.shuffle(data, _dca_mapper, target=target,
                         kw={'labels': labels, 'alpha': alpha, 'w': w_host, 'scaled_lambda': scaled_lambda,
                             'chains': chains}).evaluate()
    # w = expr.sum(data * alpha * 1.0 / la / data.shape[0], axis=0).reshape((data.shape[1], 1))
    w = expr.reshape(expr.sum(expr.lazify(data) * expr.lazify(alpha) * one / la_t / n_t, axis=0), (d, 1))
    w = w.optimized().evaluate()
  return w, alpha


def fit(data, labels, T=50, la=1.0, dtype=None, chains_per_tile=1):
  """Train a linear SVM on `data` (expression / distributed array / NumPy array of shape (n, d)) with `labels` ((n,) or
  (n, 1), +1 or -1) by T iterations of DisDCA with the parameter lambda = `la`: the weight vector w (d, 1) in `dtype`
  (default: the data's if it is float32 or float64, float64 otherwise) as a lazy expression, as the reference returns
  it.  See the module docstring for the formulas, `chains_per_tile` and the errors."""
  return expr.lazify(fit_state(data, labels, T=T, la=la, dtype=dtype, chains_per_tile=chains_per_tile)[0])


def _host(a):
  return np.asarray(a) if isinstance(a, np.ndarray) else np.asarray(expr.evaluate(a).glom())


def predict(w, new_data):
  """The reference's label of ONE instance `new_data` ((d,) or (1, d)): 1 if np.dot(new_data, w) >= 0, else -1."""
  ret = np.dot(_host(new_data), _host(w))
  if ret >= 0:
    return 1
  return -1


def predict_labels(w, data):
  """The label of every row of `data` (n, d): an expression of shape (n, 1), int64, +1 where dot(data, w) >= 0 and -1
  elsewhere."""
  if isinstance(data, np.ndarray):
    data = expr.from_numpy(data)
  if isinstance(w, np.ndarray):
    w = expr.from_numpy(w)
  if len(data.shape) != 2 or tuple(w.shape) != (data.shape[1], 1):
    raise ValueError('predict_labels: data of shape %s for a w of shape %s' % (tuple(data.shape), tuple(w.shape)))
  data, w = expr.evaluate(data), expr.evaluate(w)
  if np.dtype(data.dtype) != np.dtype(w.dtype):
    data = expr.astype(data, w.dtype)
  scores = expr.dot(data, w)
  return expr.astype(expr.greater_equal(scores, np.dtype(w.dtype).type(0)), np.int64) * np.int64(2) - np.int64(1)
