"""Blocked Cholesky factorisation of a distributed matrix (interface of the reference's spartan/examples/cholesky.py:
`cholesky(A)` -> the lower factor L with A = L . L^T, zero above the diagonal).

The row tiles of A are read as a g x g grid of cells, g = floor(sqrt(num_workers)) (map2's region join,
expr/map.region_join_mapper).  Step k of g:
  1. the diagonal cell (k, k) is factored                         potrf      (sp_potrf on the HIP backend)
  2. the cells below it are solved against that factor            trsm_rlt   (sp_trsm_rlt)
  3. every cell (l, m), k < m <= l, gives up A_lk . A_mk^T          the backend's dot (the MFMA GEMM) and a fused subtract
and a last pass zeroes the cells above the diagonal.  Step 3 takes the full product on diagonal cells as well:
potrf reads their lower half only.  Each step is one map2(..., update_region=...) over the whole array, as in the
reference; cells outside the region pass through unchanged.
"""
import math

from .. import context, expr
from ..array import extent
from . import _dense


def _potrf_mapper(extents, tiles):
  return extents[0], _dense.potrf(tiles[0])


def _trsm_mapper(extents, tiles):
  # tiles[1]: the whole factored diagonal cell (its join axis is None)
  return extents[0], _dense.trsm_rlt(tiles[0], tiles[1])


def _update_mapper(extents, tiles):
  # tiles[1]: columns of the transposed panel under the cell's ROW range, i.e. A_lk^T; tiles[2]: rows of the panel
  # under the cell's COLUMN range, A_mk
  return extents[0], tiles[0] - tiles[1].T.dot(tiles[2].T)


def _zero_mapper(extents, tiles):
  return extents[0], 0


def _whole_mapper(extents, tiles):
  yield extents[0], _dense.potrf(tiles[0])


_whole_mapper.yields_fresh_tensors = True      # the factor is a new tensor, never the fetched tile


def _box(ul, lr, shape):
  return extent.create(ul, lr, shape)


def cholesky(A):
  """L, lower triangular with A = L . L^T, for a symmetric positive definite matrix expression `A` whose order is a
  multiple of floor(sqrt(num_workers)) (1, or 4 and more workers); the dtype (float32 or float64) and shape of A.  numpy.linalg.LinAlgError if A
  is not positive definite."""
  shape = tuple(A.shape)
  if len(shape) != 2 or shape[0] != shape[1]:
    raise ValueError('cholesky: expected a square matrix, got shape %s' % (shape,))
  g = max(1, int(math.sqrt(context.get().num_workers)))
  if shape[0] % g:
    raise ValueError('cholesky: order %d is not a multiple of the grid side %d' % (shape[0], g))
  if g == 1:                     # one cell: the region join has no grid to map an untiled array onto
    if context.get().num_workers != 1:
      raise ValueError('cholesky: 2 or 3 workers make no square grid of cells; use 1, or 4 and more')
    return expr.map2(A, (0,), fn=_whole_mapper, shape=shape, tile_hint=shape)
  step = shape[0] // g
  cells = (step, step)
  for k in range(g):
    lo, hi = k * step, (k + 1) * step
    diag = _box((lo, lo), (hi, hi), shape)
    A = expr.map2(A, ((0, 1),), fn=_potrf_mapper, shape=shape, update_region=diag)
    if k == g - 1:
      break
    below = _box((hi, lo), (g * step, hi), shape)
    A = expr.map2((A, A[diag.to_slice()]), ((0, 1), None), fn=_trsm_mapper, shape=shape, update_region=below)
    panel = A[:, lo:hi]
    trailing = [_box((m * step, m * step), (g * step, (m + 1) * step), shape) for m in range(k + 1, g)]
    # (left as built, not .optimized(): the optimizer's rewrite of this step leaves the solve's result in the default
    # row tiles, and row tiles of uneven height -- 192 rows on 9 workers -- do not number onto the grid of cells)
    A = expr.map2((A, expr.transpose(panel), panel), ((0, 1), 1, 0), fn=_update_mapper, shape=shape,
                  update_region=trailing)
  above = [_box((0, m * step), (m * step, (m + 1) * step), shape) for m in range(1, g)]
  return expr.map2(A, ((0, 1),), fn=_zero_mapper, shape=shape, update_region=above)
