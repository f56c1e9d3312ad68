"""The tile bodies of the item recommender: backend.item_topk / backend.item_topk_merge where the backend has them
(HipBackend: sp_item_topk / sp_item_topk_merge), NumPy on host arrays otherwise -- the same arithmetic in the same order
(include/spartan_hip_cf.h), which keeps the driver runnable on a backend of plain NumPy tiles.  Both paths refuse
through one function, tile_checks.check_item_topk_operands (the launcher and HipBackend.item_topk call it too)."""
import functools

import numpy as np

from ... import context, tile_checks
from ...array import distarray
from .._select import select

check_operands = tile_checks.check_item_topk_operands
_select = functools.partial(select, largest=True)


def similarities_numpy(targets, tnorm, sources, snorm):
  """[m, ns] in the operands' dtype T: sim[j][i] as the kernel forms it -- one accumulator per pair that starts at 0 and
  takes t[u][j] * s[u][i] for u = 0, 1, ... in turn (one user after the other, vectorised over the pairs), one product
  of norms, one division, nan_to_num."""
  dt = targets.dtype
  dot = np.zeros((targets.shape[1], sources.shape[1]), dt)
  with np.errstate(all='ignore'):
    for u in range(targets.shape[0]):
      dot = dot + targets[u][:, None] * sources[u][None, :]
    sim = np.nan_to_num(dot / (tnorm[:, None] * snorm[None, :]))
  assert sim.dtype == dt
  return sim


def item_topk_numpy(targets, tnorm, sources, snorm, k, index_offset=0):
  """item_topk on host arrays."""
  sim = similarities_numpy(targets, tnorm, sources, snorm)
  idx = np.broadcast_to(np.arange(sources.shape[1], dtype=np.int64) + int(index_offset), sim.shape)
  return _select(sim, idx, np.ones(sim.shape, bool), int(k))


def _absent_pair(m, k, dtype):
  return distarray.Absent((m, k), dtype), distarray.Absent((m, k), np.int64)


def item_topk(targets, tnorm, sources, snorm, k, index_offset=0, splits=0):
  """(sim, idx) as new tiles [m, k]: for every column of the tile `targets` [users, m] the k columns of `sources`
  [users, ns] of the largest cosine similarity, ordered by (similarity descending, index ascending), idx = index_offset +
  column; -inf / -1 where the tile has fewer than k columns.  tnorm [m], snorm [ns]: the columns' norms.  TypeError
  ("astype first") for other or mixed dtypes, ValueError for shapes that do not fit, a k outside 1 .. 128 or
  splits < 0."""
  operands = (targets, tnorm, sources, snorm)
  if any(isinstance(t, distarray.Absent) for t in operands):
    dt, _, m, _, k, _ = check_operands([t.dtype for t in operands], targets.shape, tnorm.shape, sources.shape,
                                       snorm.shape, k, splits)
    return _absent_pair(m, k, dt)
  be = context.get().backend
  fn = getattr(be, 'item_topk', None)
  if fn is not None:
    return fn(targets, tnorm, sources, snorm, k, index_offset=index_offset, splits=splits)
  t, tn, s, sn = (np.asarray(be.to_numpy(a)) for a in operands)
  _, _, _, _, k, _ = check_operands([a.dtype for a in (t, tn, s, sn)], t.shape, tn.shape, s.shape, sn.shape, k, splits)
  return item_topk_numpy(t, tn, s, sn, k, index_offset)


def item_topk_merge(cand_sim, cand_idx, k):
  """(sim, idx), both [m, k]: per row the k best by (similarity descending, index ascending) of the candidates; those
  with a negative index are padding."""
  if isinstance(cand_sim, distarray.Absent) or isinstance(cand_idx, distarray.Absent):
    return _absent_pair(cand_sim.shape[0], k, cand_sim.dtype)
  be = context.get().backend
  fn = getattr(be, 'item_topk_merge', None)
  if fn is not None:
    return fn(cand_sim, cand_idx, k)
  sim, idx = np.asarray(be.to_numpy(cand_sim)), np.asarray(be.to_numpy(cand_idx))
  k = tile_checks.check_item_topk_merge((sim.dtype, idx.dtype), (sim.shape, idx.shape), k)[3]
  return _select(sim, idx, (idx >= 0) & ~np.isnan(sim), k)
