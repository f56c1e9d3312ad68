"""Naive Bayes on tf-idf weights (interface of the reference's spartan/examples/naive_bayes.py: `fit(data, labels,
label_size, alpha)` -> the model dict, `predict(model, new_data)` -> a label).

fit, with data [n, d] documents x terms and labels [n] or [n, 1] (naive_bayes.py:26-79):

    df_j  = the documents with x_ij > 0               idf_j = log(n / (df_j + 1)) + 1
    r_i   = sqrt(sum_j x_ij^2 / d)                    z_ij  = x_ij / r_i
    W_lj  = idf_j * sum over the documents of label l of z_ij        wl_l = sum_j W_lj
    scores_lj = log((W_lj + alpha) / (wl_l + alpha d))

The reference makes five passes over the data, three of them maps that write an n x d array, and then adds the rows to
their labels one interpreted step per document.  Here ONE shuffle over the row bands calls _nb.nb_step on each
(HipBackend: sp_nb_step -- normalisation, label sums and df fused, nothing of size n x d allocated) and updates three
single-tile targets: S (label_size, d) and df (d,), both with reduce_fn=np.add, and a slot per band for the band's
first label out of range.  idf is constant over a column, so it multiplies the summed S afterwards (another rounding
than the reference's `* idf` inside the sum, the same mathematics); the rest are expressions on the map and reduce
kernels.

Behaviour of the reference that is kept: a document without a term has r = 0 and turns its label's row of the
scores into NaN; 'scores_per_label' is the un-logged wl (the reference's name).

Deviations: `data` may be float32 (the run is then in float32; integer counts are converted to float64 on the device;
`dtype` forces either); integer labels of another width are converted to int64, float labels raise TypeError; a label
outside 0 .. label_size - 1 raises IndexError naming the row (NumPy would wrap a negative one); alpha not finite or
<= 0, label_size outside 1 .. 128, data that is not 2-D and labels that are not of n rows raise ValueError;
`predict_labels` is an addition."""
import numpy as np

from .. import _hip, context, expr, tile_checks
from ..array import distarray, extent
from . import _nb

_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def _fit_mapper(inputs, ex, data, labels, label_size, dtype, slots, sums, df, bad):
  """Tile body of fit: the step of one row band, pushed into the three targets."""
  if ex.ul[1] != 0:                     # (a band cut by columns as well: its first tile speaks for all of them)
    return []
  be = context.get().backend
  lo, hi = ex.ul[0], ex.lr[0]
  x = data.fetch(extent.create((lo, 0), (hi, data.shape[1]), data.shape))
  if len(labels.shape) == 2:
    y = labels.fetch(extent.create((lo, 0), (hi, 1), labels.shape))
  else:
    y = labels.fetch(extent.create((lo,), (hi,), labels.shape))
  if not isinstance(x, distarray.Absent):
    x = be.astype(x, dtype)
  tile_s, tile_df, tile_bad = _nb.nb_step(x, y, label_size)
  sums.update(extent.from_shape(sums.shape), tile_s)
  df.update(extent.from_shape(df.shape), tile_df)
  slot = slots[lo]
  bad.update(extent.create((slot,), (slot + 1,), bad.shape), tile_bad)
  return []


def fit(data, labels, label_size, alpha=1.0, dtype=None):
  """The model of `data` (expression / distributed array / NumPy array of shape (n, d), tiled by rows) with `labels`
  ((n,) or (n, 1), integers in 0 .. label_size - 1): {'scores_per_label_and_feature': (label_size, d),
  'scores_per_label': (label_size,)}, evaluated distributed arrays in `dtype` (default: the data's if it is float32 or
  float64, float64 otherwise).  See the module docstring for the formulas, the special values and the errors."""
  alpha = tile_checks.check_finite_positive('fit: alpha', alpha)
  label_size = int(label_size)
  if not 1 <= label_size <= _hip.SP_NB_MAX_LABELS:
    raise ValueError('fit: label_size = %d must be in 1 .. %d' % (label_size, _hip.SP_NB_MAX_LABELS))
  if isinstance(data, np.ndarray):
    data = expr.from_numpy(data)
  if isinstance(labels, np.ndarray):
    labels = expr.from_numpy(labels)
  if len(data.shape) != 2:
    raise ValueError('fit: expected data of shape (n, d), got %s' % (tuple(data.shape),))
  n, d = (int(v) for v in data.shape)
  if tuple(int(v) for v in labels.shape) not in ((n,), (n, 1)):
    raise ValueError('fit: labels of shape %s for %d rows' % (tuple(labels.shape), n))
  data, labels = expr.evaluate(data), expr.evaluate(labels)
  if np.dtype(labels.dtype).kind not in 'iub':
    raise TypeError('fit: labels of dtype %s; the labels are integers' % np.dtype(labels.dtype))
  if dtype is None:
    dtype = np.dtype(data.dtype) if np.dtype(data.dtype) in _FLOATS else np.dtype(np.float64)
  dtype = tile_checks.check_float_dtype(dtype, 'fit')
  if np.dtype(labels.dtype) != np.int64:
    labels = expr.evaluate(expr.astype(labels, np.int64))

  slots = {lo: i for i, lo in enumerate(sorted(set(ex.ul[0] for ex in data.tiles if ex.ul[1] == 0)))}
  nslots = max(len(slots), 1)
  sums = expr.ndarray((label_size, d), dtype=dtype, reduce_fn=np.add, tile_hint=(label_size, d))
  df = expr.ndarray((d,), dtype=np.int64, reduce_fn=np.add, tile_hint=(d,))
  bad = expr.ndarray((nslots,), dtype=np.int64, tile_hint=(nslots,))
  expr.shuffle(data, _fit_mapper,
               kw={'data': data, 'labels': labels, 'label_size': label_size, 'dtype': dtype, 'slots': slots,
                   'sums': sums, 'df': df, 'bad': bad},
               shape_hint=(1,)).evaluate()
  if slots:
    first = np.asarray(bad.glom()).reshape(-1)
    for lo, slot in sorted(slots.items()):
      if first[slot]:
        row = lo + int(first[slot]) - 1
        raise IndexError('fit: the label of row %d is outside 0 .. %d' % (row, label_size - 1))

  one = dtype.type(1)
  idf = expr.log(dtype.type(n) / (expr.astype(df, dtype) + one)) + one
  weights = sums * expr.reshape(idf, (1, d))
  weights_per_label = expr.sum(weights, axis=1)
  scores = expr.log((weights + dtype.type(alpha))
                    / (expr.reshape(weights_per_label, (label_size, 1)) + dtype.type(alpha * d)))
  return {'scores_per_label_and_feature': scores.optimized().evaluate(),
          'scores_per_label': weights_per_label.optimized().evaluate()}


def _scores_and(model, new_data):
  scores = model['scores_per_label_and_feature']
  if isinstance(new_data, np.ndarray):
    new_data = expr.from_numpy(new_data)
  if len(new_data.shape) != 2 or new_data.shape[1] != scores.shape[1]:
    raise ValueError('predict: data of shape %s for a model of %d features' % (tuple(new_data.shape), scores.shape[1]))
  new_data = expr.evaluate(new_data)
  if np.dtype(new_data.dtype) != np.dtype(scores.dtype):
    new_data = expr.astype(new_data, scores.dtype)
  return scores, new_data


def predict(model, new_data):
  """The reference's np.argmax(dot(scores, transpose(new_data)).glom()): for `new_data` of ONE row (1, d), the label
  with the largest score.  For more rows it is what the reference computes -- the arg-max over the flattened
  (label_size, rows) product, i.e. label * rows + row of the single best pair -- and hardly what a caller wants:
  predict_labels gives a label per row."""
  scores, new_data = _scores_and(model, new_data)
  return np.argmax(np.asarray(expr.dot(scores, expr.transpose(new_data)).glom()))


def predict_labels(model, data):
  """The label of every row of `data` (n, d): an expression of shape (n,), int64, the arg-max over the labels (the
  lowest at a tie) of dot(data, transpose(scores))."""
  scores, data = _scores_and(model, data)
  return expr.argmax(expr.dot(data, expr.transpose(scores)), axis=1)
