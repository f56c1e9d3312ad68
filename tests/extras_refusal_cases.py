"""What the tile bodies outside the fused path refuse, as one table: per operation the smallest valid call, what its
check function (spartan_amd/tile_checks.py) returns for it, what the call returns, and one row per condition the
operation refuses -- (what to break, the class, a fragment of the text).

The classes and fragments were read off HipBackend.<op> as it stood before the checks were gathered in tile_checks.py
(the commit "Split-tier GEMM: read the next k-tile's fragments under the MFMAs"), not off the code under test: every path
(the check function, the NumPy body under examples/, HipBackend.<op>, the launcher kernels.<op>) has to raise them.

A call is the list of the arguments of HipBackend.<op> in the order of its signature; the NumPy body takes a prefix of
them (it has no `splits` where the recipe has no ranges), and a defect in an argument a path does not take is not run
through that path.  tests/test_extras_refusals_cpu.py and tests/test_extras_refusals_gpu.py run the table.
"""
import collections

import numpy as np

from spartan_amd import tile_checks as tc

F64, F32, I64 = np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.int64)


def reals(*shape):
  """Positive float64 values in (0, 2), every one different."""
  n = int(np.prod(shape))
  return (((np.arange(n, dtype=np.float64) * 7) % 11 + 1) / 6.5 + np.arange(n) / (16.0 * max(n, 1))).reshape(shape)


def indices(rows, cols, below):
  return ((np.arange(rows * cols, dtype=np.int64) * 5 + 1) % below).reshape(rows, cols)


def _dt(*arrays):
  return [a.dtype for a in arrays if a is not None]


def _sh(*arrays):
  return [a.shape for a in arrays if a is not None]


# (argument index, its replacement) ... -> the broken call
def _cast(i, dtype):
  return lambda a: a[:i] + [a[i].astype(dtype)] + a[i + 1:]


def _put(i, value):
  return lambda a: a[:i] + [value] + a[i + 1:]


# body: 'module:function' of the NumPy dispatcher; check(call) -> the check function's answer; sizes: that answer for the
# valid call; results: (shape, dtype) of what the valid call returns; launch(kernels, call, targets): the launcher on the
# same operands, targets = one device array per result and a one-element int32 `info` last (None: no such launcher)
Op = collections.namedtuple('Op', 'name body valid check sizes results defects launch')
# arg: the index of the argument that make(call) breaks
Defect = collections.namedtuple('Defect', 'label arg make cls fragment')


BY_BACKEND = 'dtype %%s is not supported by %s of the HIP tile backend'      # _hip.refuse_not_float's words
BY_CHECK = '%s: dtype %%s is not supported (float32 float64)'                # the words of the three newest families


def _dtype_rows(text, operands):
  """int32 and float16 in the place of every float operand."""
  return [('arg%d %s' % (i, bad), i, _cast(i, bad), TypeError, text % bad) for i in operands for bad in ('int32', 'float16')]


def _defects(rows):
  return [Defect(*r) for r in rows]


_SPD = reals(9, 3).T.dot(reals(9, 3)) + np.eye(3)
_LOW = np.tril(reals(3, 3)) + np.eye(3)
_X = reals(9, 3)
_SQUARE = [('shape 9x3', 0, _put(0, reals(9, 3)), ValueError, '%s: expected a square matrix, got shape (9, 3)'),
           ('1-D', 0, _put(0, reals(9)), ValueError, '%s: expected a square matrix, got shape (9,)')]


def _square_op(name, body, valid, results, launch):
  rows = _dtype_rows(BY_BACKEND % name, (0,)) + [(l, i, m, c, f % name) for l, i, m, c, f in _SQUARE]
  check = getattr(tc, 'check_' + name)
  return Op(name, body, [valid], lambda a: check(a[0].dtype, a[0].shape), (F64, 3), results, _defects(rows), launch)


def _merge_op(name, body, check):
  rows = _dtype_rows(BY_BACKEND % name, (0,)) + [
      ('idx int32', 1, _cast(1, 'int32'), TypeError, '%s: candidate indices of dtype int32 (int64 expected)' % name),
      ('shapes', 1, _put(1, indices(9, 3, 9)), ValueError, '%s: shapes (9, 4) and (9, 3) do not fit' % name),
      ('1-D', 0, _put(0, reals(9)), ValueError, '%s: shapes (9,) and (9, 4) do not fit' % name),
      ('k = 0', 2, _put(2, 0), ValueError, '%s: k = 0 is outside 1 .. 128' % name),
      ('k = 129', 2, _put(2, 129), ValueError, '%s: k = 129 is outside 1 .. 128' % name)]
  return Op(name, body, [reals(9, 4), indices(9, 4, 30), 2], lambda a: check(_dt(*a[:2]), _sh(*a[:2]), a[2]), (F64, 9, 4, 2),
            [((9, 2), F64), ((9, 2), I64)], _defects(rows),
            lambda k, a, t: getattr(k, name)(a[0], a[1], a[2], t[0], t[1]))


def _affinity_params(name, metric, gamma):
  """What check_affinity_params refuses, for the call whose arguments `metric` and `gamma` are the metric and gamma."""
  return [
      ('unknown metric', metric, _put(metric, 'cosine'), ValueError, "%s: unknown metric 'cosine'" % name),
      ('scaled_euclidean', metric, _put(metric, 'scaled_euclidean'), NotImplementedError,
       "%s: 'scaled_euclidean' is refused" % name),
      ('gamma nan', gamma, _put(gamma, float('nan')), ValueError, '%s: gamma = nan must be finite' % name),
      ('gamma inf', gamma, _put(gamma, float('inf')), ValueError, '%s: gamma = inf must be finite' % name)]


OPS = [
    _square_op('potrf', 'spartan_amd.examples._dense:potrf', _SPD, [((3, 3), F64)],
               lambda k, a, t: k.potrf(a[0], t[-1])),
    Op('trsm_rlt', 'spartan_amd.examples._dense:trsm_rlt', [_X, _LOW],
       lambda a: tc.check_trsm_rlt(_dt(*a), _sh(*a)), (F64, 9, 3), [((9, 3), F64)],
       _defects(_dtype_rows(BY_BACKEND % 'trsm_rlt', (0, 1)) + [
           ('mixed', 0, _cast(0, 'float32'), TypeError, 'trsm_rlt: operands of two dtypes (float32, float64)'),
           ('l 4x4', 1, _put(1, reals(4, 4)), ValueError, 'trsm_rlt: shapes (9, 3) and (4, 4) do not fit'),
           ('l 3x4', 1, _put(1, reals(3, 4)), ValueError, 'trsm_rlt: shapes (9, 3) and (3, 4) do not fit'),
           ('b 1-D', 0, _put(0, reals(3)), ValueError, 'trsm_rlt: shapes (3,) and (3, 3) do not fit')]),
       lambda k, a, t: k.trsm_rlt(a[0], a[1])),
    _square_op('syev', 'spartan_amd.examples._dense:syev', _SPD, [((3,), F64), ((3, 3), F64)], None),
    Op('knn', 'spartan_amd.examples.sklearn.neighbors._knn:knn', [_X, reals(9, 3)[::-1].copy(), 2, 0, 0],
       lambda a: tc.check_knn(_dt(*a[:2]), _sh(*a[:2]), a[2], a[4]), (F64, 9, 9, 3, 2, 0), [((9, 2), F64), ((9, 2), I64)],
       _defects(_dtype_rows(BY_BACKEND % 'knn', (0, 1)) + [
           ('mixed', 0, _cast(0, 'float32'), TypeError, 'knn: operands of two dtypes (float32, float64)'),
           ('points 9x4', 1, _put(1, reals(9, 4)), ValueError, 'knn: shapes (9, 3) and (9, 4) do not fit'),
           ('queries 1-D', 0, _put(0, reals(3)), ValueError, 'knn: shapes (3,) and (9, 3) do not fit'),
           ('k = 0', 2, _put(2, 0), ValueError, 'knn: k = 0 is outside 1 .. 128'),
           ('k = 129', 2, _put(2, 129), ValueError, 'knn: k = 129 is outside 1 .. 128'),
           ('splits = -1', 4, _put(4, -1), ValueError, 'knn: splits = -1 is negative')]),
       lambda k, a, t: k.knn(a[0], a[1], a[2], t[0], t[1], a[3], a[4])),
    _merge_op('knn_merge', 'spartan_amd.examples.sklearn.neighbors._knn:knn_merge', tc.check_knn_merge),
    Op('item_topk', 'spartan_amd.examples.cf._cf:item_topk',
       [_X, np.sqrt((_X * _X).sum(axis=0)), reals(9, 4), np.sqrt((reals(9, 4) ** 2).sum(axis=0)), 2, 0, 0],
       lambda a: tc.check_item_topk_operands(_dt(*a[:4]), a[0].shape, a[1].shape, a[2].shape, a[3].shape, a[4], a[6]),
       (F64, 9, 3, 4, 2, 0), [((3, 2), F64), ((3, 2), I64)],
       _defects(_dtype_rows(BY_CHECK % 'item_topk', (0, 1, 2, 3)) + [
           ('mixed', 2, _cast(2, 'float32'), TypeError, 'item_topk: operands of two dtypes (float64, float32)'),
           ('targets 1-D', 0, _put(0, reals(9)), ValueError, 'item_topk: targets and sources must be 2-D [users, items]'),
           ('users', 2, _put(2, reals(8, 4)), ValueError, 'item_topk: targets of 9 users against sources of 8'),
           ('tnorm', 1, _put(1, reals(4)), ValueError, 'item_topk: norms of shapes (4,) and (4,) for 3 targets and 4 sources'),
           ('k = 0', 4, _put(4, 0), ValueError, 'item_topk: k = 0 is outside 1 .. 128'),
           ('k = 129', 4, _put(4, 129), ValueError, 'item_topk: k = 129 is outside 1 .. 128'),
           ('splits = -1', 6, _put(6, -1), ValueError, 'item_topk: splits = -1 is negative')]),
       lambda k, a, t: k.item_topk(a[0], a[1], a[2], a[3], a[4], t[0], t[1], a[5], a[6])),
    _merge_op('item_topk_merge', 'spartan_amd.examples.cf._cf:item_topk_merge', tc.check_item_topk_merge),
    _square_op('apsp', 'spartan_amd.examples.sklearn.manifold._graph:apsp', reals(3, 3), [((3, 3), F64)],
               lambda k, a, t: k.apsp(a[0], t[-1])),
    Op('graph_from_knn', 'spartan_amd.examples.sklearn.manifold._graph:graph_from_knn', [reals(9, 2), indices(9, 2, 9)],
       lambda a: tc.check_graph_from_knn(_dt(*a), _sh(*a)), (F64, 9, 2), [((9, 9), F64)],
       _defects(_dtype_rows(BY_BACKEND % 'graph_from_knn', (0,)) + [
           ('idx int32', 1, _cast(1, 'int32'), TypeError, 'graph_from_knn: indices of dtype int32 (int64 expected)'),
           ('shapes', 1, _put(1, indices(9, 3, 9)), ValueError, 'graph_from_knn: shapes (9, 2) and (9, 3) do not fit'),
           ('1-D', 0, _put(0, reals(9)), ValueError, 'graph_from_knn: shapes (9,) and (9, 2) do not fit')]),
       lambda k, a, t: k.graph_from_knn(a[0], a[1], t[0])),
    Op('als_solve', 'spartan_amd.examples._als:als_solve', [_X, reals(3, 2), 0.1, 1.0, False, None],
       lambda a: tc.check_als_solve(_dt(*a[:2]), _sh(*a[:2])), (F64, 9, 3, 2), [((9, 2), F64)],
       _defects(_dtype_rows(BY_BACKEND % 'als_solve', (0, 1)) + [
           ('mixed', 0, _cast(0, 'float32'), TypeError, 'als_solve: operands of two dtypes (float32, float64)'),
           ('factors 4x2', 1, _put(1, reals(4, 2)), ValueError, 'als_solve: shapes (9, 3) and (4, 2) do not fit'),
           ('ratings 1-D', 0, _put(0, reals(3)), ValueError, 'als_solve: shapes (3,) and (3, 2) do not fit'),
           ('f = 0', 1, _put(1, reals(3, 0)), ValueError, 'als_solve: f = 0 is outside 1 .. 64'),
           ('f = 65', 1, _put(1, reals(3, 65)), ValueError, 'als_solve: f = 65 is outside 1 .. 64')]),
       lambda k, a, t: k.als_solve(a[0], a[1], a[2], a[3], a[4], t[0], t[-1])),
    Op('fuzzy_step', 'spartan_amd.examples._fuzzy:fuzzy_step', [_X, reals(2, 3), 2.0, False, 0],
       lambda a: tc.check_fuzzy_step(_dt(*a[:2]), _sh(*a[:2]), a[2], a[4]), (F64, 9, 2, 3, 2.0, 0),
       [((9,), I64), ((2, 3), F64), ((2,), F64)],
       _defects(_dtype_rows(BY_BACKEND % 'fuzzy_step', (0, 1)) + [
           ('mixed', 1, _cast(1, 'float32'), TypeError, 'fuzzy_step: operands of two dtypes (float64, float32)'),
           ('m = 1', 2, _put(2, 1), ValueError, 'fuzzy_step: m = 1.0 must be finite and > 1'),
           ('m = inf', 2, _put(2, float('inf')), ValueError, 'fuzzy_step: m = inf must be finite and > 1'),
           ('m = nan', 2, _put(2, float('nan')), ValueError, 'fuzzy_step: m = nan must be finite and > 1'),
           ('centers 2x4', 1, _put(1, reals(2, 4)), ValueError, 'fuzzy_step: shapes (9, 3) and (2, 4) do not fit'),
           ('points 1-D', 0, _put(0, reals(3)), ValueError, 'fuzzy_step: shapes (3,) and (2, 3) do not fit'),
           ('k = 0', 1, _put(1, reals(0, 3)), ValueError, 'fuzzy_step: k = 0 must be at least 1'),
           ('splits = -1', 4, _put(4, -1), ValueError, 'fuzzy_step: splits = -1')]),
       lambda k, a, t: k.fuzzy_step(a[0], a[1], a[2], t[0], t[1], t[2], None, a[4])),
    Op('lda_step', 'spartan_amd.examples._lda:lda_step', [_X, reals(2, 9), 0.1, 0.2, 2, True, True, 0],
       lambda a: tc.check_lda_step(_dt(*a[:2]), _sh(*a[:2]), a[2], a[3], a[4], a[7]), (F64, 9, 3, 2, 0.1, 0.2, 2, 0),
       [((2, 9), F64), ((3, 2), F64)],
       _defects(_dtype_rows(BY_BACKEND % 'lda_step', (0, 1)) + [
           ('mixed', 0, _cast(0, 'float32'), TypeError, 'lda_step: operands of two dtypes (float32, float64)'),
           ('n 2x8', 1, _put(1, reals(2, 8)), ValueError, 'lda_step: shapes (9, 3) and (2, 8) do not fit'),
           ('x 1-D', 0, _put(0, reals(9)), ValueError, 'lda_step: shapes (9,) and (2, 9) do not fit'),
           ('k = 0', 1, _put(1, reals(0, 9)), ValueError, 'lda_step: k = 0 must be in 1 .. 128'),
           ('k = 129', 1, _put(1, reals(129, 9)), ValueError, 'lda_step: k = 129 must be in 1 .. 128'),
           ('iters = 0', 4, _put(4, 0), ValueError, 'lda_step: iters = 0 must be at least 1'),
           ('alpha = 0', 2, _put(2, 0), ValueError, 'lda_step: alpha = 0.0 must be finite and > 0'),
           ('alpha = inf', 2, _put(2, float('inf')), ValueError, 'lda_step: alpha = inf must be finite and > 0'),
           ('eta = 0', 3, _put(3, 0), ValueError, 'lda_step: eta = 0.0 must be finite and > 0'),
           ('eta = nan', 3, _put(3, float('nan')), ValueError, 'lda_step: eta = nan must be finite and > 0'),
           ('splits = -1', 7, _put(7, -1), ValueError, 'lda_step: splits = -1')]),
       lambda k, a, t: k.lda_step(a[0], a[1], a[2], a[3], a[4], t[0], t[1], a[7])),
    Op('nb_step', 'spartan_amd.examples._nb:nb_step', [_X, indices(9, 1, 2).reshape(9), 2, 0],
       lambda a: tc.check_nb_operands(a[0].dtype, a[0].shape, a[1].dtype, a[1].shape, a[2], a[3]), (9, 3, 2),
       [((2, 3), F64), ((3,), I64), ((1,), I64)],
       _defects(_dtype_rows(BY_CHECK % 'nb_step', (0,)) + [
           ('labels int32', 1, _cast(1, 'int32'), TypeError, 'nb_step: labels of dtype int32; convert with astype(int64) first'),
           ('label_size = 0', 2, _put(2, 0), ValueError, 'nb_step: label_size = 0 must be in 1 .. 128'),
           ('label_size = 129', 2, _put(2, 129), ValueError, 'nb_step: label_size = 129 must be in 1 .. 128'),
           ('x 1-D', 0, _put(0, reals(9)), ValueError, 'nb_step: expected data of shape (m, d), got (9,)'),
           ('labels 8', 1, _put(1, indices(8, 1, 2).reshape(8)), ValueError, 'nb_step: labels of shape (8,) for 9 rows'),
           ('splits = -1', 3, _put(3, -1), ValueError, 'nb_step: splits = -1')]),
       lambda k, a, t: k.nb_step(a[0], a[1], a[2], t[0], t[1], t[2], a[3])),
    Op('nbody_accel', 'spartan_amd.examples._nbody:nbody_accel',
       [reals(9), reals(9)[::-1].copy(), reals(9) * 3, reals(9) + 1, 2, 4, 1.0, 1.0, 0],
       lambda a: tc.check_nbody_operands(_dt(*a[:4]), _sh(*a[:4]), *a[4:]), (F64, 9, 2, 4, 1.0, 1.0, 0),
       [((4,), F64)] * 3,
       _defects(_dtype_rows(BY_CHECK % 'nbody_accel', (0, 1, 2, 3)) + [
           ('mixed', 3, _cast(3, 'float32'), TypeError, 'nbody_accel: operands of two dtypes (float64, float32)'),
           ('z 8', 2, _put(2, reals(8)), ValueError, 'nbody_accel: x, y, z and mass must be 1-D and of equal length'),
           ('r0 + m > n', 4, _put(4, 6), ValueError, 'nbody_accel: bodies 6 .. 10 are not among the 9'),
           ('r0 = -1', 4, _put(4, -1), ValueError, 'nbody_accel: bodies -1 .. 3 are not among the 9'),
           ('splits = -1', 8, _put(8, -1), ValueError, 'nbody_accel: splits = -1'),
           ('g = nan', 6, _put(6, float('nan')), ValueError, 'nbody_accel: g = nan must be finite in float64'),
           ('g = inf', 6, _put(6, float('inf')), ValueError, 'nbody_accel: g = inf must be finite in float64'),
           ('rmin = 0', 7, _put(7, 0), ValueError, 'nbody_accel: rmin = 0.0 must be finite and > 0 in float64'),
           ('rmin = inf', 7, _put(7, float('inf')), ValueError, 'nbody_accel: rmin = inf must be finite and > 0 in float64')]),
       lambda k, a, t: k.nbody_accel(a[0], a[1], a[2], a[3], a[4], a[5], t[0], t[1], t[2], a[6], a[7], a[8])),
    Op('affinity_degree', 'spartan_amd.examples._spectral:affinity_degree', [_X, reals(9, 3)[::-1].copy(), 'rbf', 1.0],
       lambda a: tc.check_affinity_degree(_dt(*a[:2]), _sh(*a[:2]), a[2], a[3]), (F64, 9, 9, 3, 0, 1.0), [((9,), F64)],
       _defects(_dtype_rows(BY_BACKEND % 'affinity_degree', (0, 1)) + [
           ('mixed', 1, _cast(1, 'float32'), TypeError, 'affinity_degree: operands of two dtypes (float64, float32)'),
           ('y 9x4', 1, _put(1, reals(9, 4)), ValueError, 'affinity_degree: shapes (9, 3) and (9, 4) do not fit'),
           ('x 1-D', 0, _put(0, reals(3)), ValueError, 'affinity_degree: shapes (3,) and (9, 3) do not fit')]
           + _affinity_params('affinity_degree', 2, 3)),
       lambda k, a, t: k.affinity_degree(a[0], a[1], a[2], a[3], t[0])),
    Op('affinity_matrix', 'spartan_amd.examples._spectral:affinity_matrix', [_X[2:6].copy(), 2, _X, 'rbf', 1.0, reals(9)],
       lambda a: tc.check_affinity_matrix(_dt(a[0], a[2], a[5]), _sh(a[0], a[2], a[5]), a[1], a[3], a[4]),
       (F64, 4, 9, 3, 0, 1.0, 2), [((4, 9), F64)],
       _defects(_dtype_rows(BY_BACKEND % 'affinity_matrix', (0, 2, 5)) + [
           ('mixed', 2, _cast(2, 'float32'), TypeError, 'affinity_matrix: operands of two dtypes (float64, float32)'),
           ('scale float32', 5, _cast(5, 'float32'), TypeError, 'affinity_matrix: operands of two dtypes (float64, float32)'),
           ('y 9x4', 2, _put(2, reals(9, 4)), ValueError, 'affinity_matrix: shapes (4, 3) and (9, 4) do not fit')]
           + _affinity_params('affinity_matrix', 3, 4) + [
           ('r0 + m > n', 1, _put(1, 6), ValueError, 'affinity_matrix: rows 6 .. 10 are not among the 9 points'),
           ('r0 = -1', 1, _put(1, -1), ValueError, 'affinity_matrix: rows -1 .. 3 are not among the 9 points'),
           ('scale 8', 5, _put(5, reals(8)), ValueError, 'affinity_matrix: a scale of shape (8,) for 9 points')]),
       lambda k, a, t: k.affinity_matrix(a[0], a[1], a[2], a[3], a[4], t[0], a[5])),
]

CASES = [(op, d) for op in OPS for d in op.defects]
CASE_IDS = ['%s-%s' % (op.name, d.label.replace(' ', '')) for op, d in CASES]


def body_of(op):
  import importlib
  module, name = op.body.split(':')
  return getattr(importlib.import_module(module), name)


def refusal(fn, *args):
  """The exception `fn(*args)` raises (None if it returns)."""
  try:
    fn(*args)
  except Exception as e:          # noqa: BLE001  (the tests compare its class and text)
    return e
  return None
