"""The selection the NumPy bodies of the nearest-neighbour and item-recommender tiles share: per row the k best
candidates in the kernels' order."""
import numpy as np

_NO_INDEX = np.iinfo(np.int64).max


def select(val, idx, valid, k, largest=False):
  """(values, indices), both [rows, k]: per row the k best of the candidates among the valid ones -- the smallest by
  (val, idx), or with `largest` the best by (val descending, idx ascending) -- padded with +inf (-inf with `largest`)
  and -1."""
  rows, cands = val.shape
  pad = -np.inf if largest else np.inf
  val = np.where(valid, val, pad).astype(val.dtype, copy=False)
  idx = np.where(valid, idx, _NO_INDEX)
  if cands < k:
    val = np.concatenate([val, np.full((rows, k - cands), pad, val.dtype)], axis=1)
    idx = np.concatenate([idx, np.full((rows, k - cands), _NO_INDEX, np.int64)], axis=1)
  order = np.lexsort((idx, -val if largest else val), axis=1)[:, :k]
  out_v = np.take_along_axis(val, order, axis=1)
  out_i = np.take_along_axis(idx, order, axis=1)
  out_i[out_i == _NO_INDEX] = -1
  return np.ascontiguousarray(out_v), np.ascontiguousarray(out_i)
