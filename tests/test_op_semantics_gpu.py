"""Every map opcode, reducer and merge reducer against NumPy at IEEE and integer edges.

The register machine of sp_interp.hpp (sp_step / sp_math) is what every element-wise expression, fused map -> reduce
and arg-reduction runs; the merge kernel (update.hip) has its own copy of the reducer rules.  Each opcode is driven
at the C-ABI level (Program + kernels.*) over an edge grid per arithmetic class, in every class the host emits it in,
on the interpreter and on the run-time specialised (hipRTC) tier, and compared with the NumPy ufunc its header
comment names on the same dtype:

* bit for bit (any NaN matches any NaN; the sign of zero must match) for everything but the transcendental opcodes;
* within ULP_BOUND ulp of a higher-precision reference for EXP, LOG, TANH, POW and NORM_CDF, with their special
  values exact;
* and the two tiers agree bit for bit on every opcode.

SEMANTICS is the table the module walks; test_semantics_table_is_complete (no GPU) fails when the header or _hip.py
grows an opcode, reducer or merge reducer that the table does not name.
"""
import math

import numpy as np
import pytest

from spartan_amd import _hip, kernels
from spartan_amd import devarray as D
from spartan_amd.program import Program, dense_strides
from tests.test_hip_kernels import _both_tiers, _interpreted, dev, host, run_reduce

F32, F64, I64 = _hip.SP_F32, _hip.SP_F64, _hip.SP_I64
CLS_DT = {F32: np.dtype(np.float32), F64: np.dtype(np.float64), I64: np.dtype(np.int64)}
CLS_V = {F32: 4, F64: 2, I64: 2}
ALL, FLT = (F32, F64, I64), (F32, F64)
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max

# DESIGN.md section c: exp / log / sqrt / div <= 2 ulp (sqrt and div are bit-exact here: IEEE correctly rounded)
ULP_BOUND = 2.0


# ------------------------------------------------------------------------------------------------- references
def _np_int_pow(a, b):
  """np.power on int64, except that NumPy raises for a negative exponent; the kernel gives 0 there (a documented
  deviation, DESIGN.md section c)."""
  neg = b < 0
  r = np.power(a, np.where(neg, 0, b))
  r[neg] = 0
  return r


def _norm_cdf(x):
  """0.5 * erfc(-x / sqrt(2)) with the argument formed as the kernel forms it (one rounding in x's precision), erfc
  itself in double precision (no SciPy)."""
  dt = x.dtype
  t = (-x) * dt.type(0.70710678118654752440)
  return np.array([0.5 * math.erfc(float(v)) for v in t.ravel()], np.float64).reshape(x.shape)


def _lnot(a):
  return np.logical_not(a)


# kind: 'exact' | 'ulp'; classes: where the host's Emitter puts the opcode (lower.py); ref(*operands) -> NumPy value
# (ref None: not a value opcode -- the test named next to it exercises it)
# arity: operands taken from registers (0: CONST / IOTA; the *C forms read one register and one constant)
SEMANTICS = {
    'NOP': dict(arity=0, classes=ALL, kind='exact', ref=None),     # skipped by the interpreter loop (every test)
    'CONST': dict(arity=0, classes=ALL, kind='exact', ref=None),   # test_const_and_iota
    'IOTA': dict(arity=0, classes=ALL, kind='exact', ref=None),    # test_const_and_iota
    'MOV': dict(arity=1, classes=ALL, kind='exact', ref=lambda a: a.copy()),
    'ADD': dict(arity=2, classes=ALL, kind='exact', ref=np.add),
    'SUB': dict(arity=2, classes=ALL, kind='exact', ref=np.subtract),
    'MUL': dict(arity=2, classes=ALL, kind='exact', ref=np.multiply),
    'DIV': dict(arity=2, classes=FLT, kind='exact', ref=np.divide),     # np.divide of integers is float64: F64 class
    'FLOORDIV': dict(arity=2, classes=ALL, kind='exact', ref=np.floor_divide),
    'MOD': dict(arity=2, classes=ALL, kind='exact', ref=np.mod),
    'FMOD': dict(arity=2, classes=ALL, kind='exact', ref=np.fmod),
    'POW': dict(arity=2, classes=ALL, kind='ulp', ref=np.power),          # I64: exact, _np_int_pow
    'MAX': dict(arity=2, classes=ALL, kind='exact', ref=np.maximum),
    'MIN': dict(arity=2, classes=ALL, kind='exact', ref=np.minimum),
    'EQ': dict(arity=2, classes=ALL, kind='exact', ref=np.equal),
    'NE': dict(arity=2, classes=ALL, kind='exact', ref=np.not_equal),
    'LT': dict(arity=2, classes=ALL, kind='exact', ref=np.less),
    'LE': dict(arity=2, classes=ALL, kind='exact', ref=np.less_equal),
    'GT': dict(arity=2, classes=ALL, kind='exact', ref=np.greater),
    'GE': dict(arity=2, classes=ALL, kind='exact', ref=np.greater_equal),
    'LAND': dict(arity=2, classes=ALL, kind='exact', ref=np.logical_and),
    'LOR': dict(arity=2, classes=ALL, kind='exact', ref=np.logical_or),
    'LXOR': dict(arity=2, classes=ALL, kind='exact', ref=np.logical_xor),
    'LNOT': dict(arity=1, classes=ALL, kind='exact', ref=_lnot),
    'NEG': dict(arity=1, classes=ALL, kind='exact', ref=np.negative),
    'ABS': dict(arity=1, classes=ALL, kind='exact', ref=np.abs),
    'SQRT': dict(arity=1, classes=FLT, kind='exact', ref=np.sqrt),
    'SQUARE': dict(arity=1, classes=ALL, kind='exact', ref=np.square),
    'EXP': dict(arity=1, classes=FLT, kind='ulp', ref=np.exp),
    'LOG': dict(arity=1, classes=FLT, kind='ulp', ref=np.log),
    'RECIP': dict(arity=1, classes=ALL, kind='exact', ref=np.reciprocal),
    'SIGN': dict(arity=1, classes=ALL, kind='exact', ref=np.sign),
    'FLOOR': dict(arity=1, classes=ALL, kind='exact', ref=np.floor),
    'CEIL': dict(arity=1, classes=ALL, kind='exact', ref=np.ceil),
    'TANH': dict(arity=1, classes=FLT, kind='ulp', ref=np.tanh),
    'NORM_CDF': dict(arity=1, classes=FLT, kind='ulp', ref=_norm_cdf),
    'WHERE': dict(arity=3, classes=ALL, kind='exact', ref=lambda c, a, b: np.where(c != 0, a, b)),
    # casts: the class value re-normalised to a narrower NumPy dtype, result kept in the class
    'TO_F32': dict(arity=1, classes=(F64,), kind='exact', ref=lambda a: a.astype(np.float32).astype(a.dtype)),
    'TO_I32': dict(arity=1, classes=ALL, kind='exact', ref=lambda a: a.astype(np.int32).astype(a.dtype)),
    'TO_I64': dict(arity=1, classes=FLT, kind='exact', ref=lambda a: a.astype(np.int64).astype(a.dtype)),
    'TO_BOOL': dict(arity=1, classes=ALL, kind='exact', ref=lambda a: a.astype(np.bool_).astype(a.dtype)),
    'TO_U8': dict(arity=1, classes=ALL, kind='exact', ref=lambda a: a.astype(np.uint8).astype(a.dtype)),
    # reg[b] (op) consts[a]
    'ADDC': dict(arity='c', classes=ALL, kind='exact', ref=np.add),
    'SUBC': dict(arity='c', classes=ALL, kind='exact', ref=np.subtract),
    'RSUBC': dict(arity='c', classes=ALL, kind='exact', ref=lambda x, c: np.subtract(c, x)),
    'MULC': dict(arity='c', classes=ALL, kind='exact', ref=np.multiply),
    'DIVC': dict(arity='c', classes=FLT, kind='exact', ref=np.divide),
    'RDIVC': dict(arity='c', classes=FLT, kind='exact', ref=lambda x, c: np.divide(c, x)),
    'MAXC': dict(arity='c', classes=ALL, kind='exact', ref=np.maximum),
    'MINC': dict(arity='c', classes=ALL, kind='exact', ref=np.minimum),
}
REDUCTIONS = {'SUM': np.sum, 'PROD': np.prod, 'MAX': np.max, 'MIN': np.min, 'AND': np.all, 'OR': np.any}
MERGE_REDUCERS = {'NONE': None, 'ADD': np.add, 'MUL': np.multiply, 'MAX': np.maximum, 'MIN': np.minimum,
                  'AND': np.logical_and, 'OR': np.logical_or}


def test_semantics_table_is_complete():
  """No GPU: the table names exactly the opcodes / reducers / merge reducers of _hip.py (and so of the header)."""
  assert set(SEMANTICS) == set(_hip.OP), sorted(set(SEMANTICS) ^ set(_hip.OP))
  assert set(REDUCTIONS) == set(_hip.RED), sorted(set(REDUCTIONS) ^ set(_hip.RED))
  assert set(MERGE_REDUCERS) == set(_hip.REDUCER), sorted(set(MERGE_REDUCERS) ^ set(_hip.REDUCER))
  import os
  import re
  hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                          'spartan_hip.h')).read()
  for prefix, names in (('SP_OP_', _hip.OP), ('SP_RED_', _hip.RED), ('SP_REDUCER_', _hip.REDUCER)):
    found = dict((m.group(1), int(m.group(2))) for m in re.finditer(r'\b%s(\w+)\s*=\s*(\d+)' % prefix, hdr))
    assert found == names, (prefix, sorted(set(found.items()) ^ set(names.items())))


# ------------------------------------------------------------------------------------------------- edge grids
def edge_grid(cls):
  rng = np.random.RandomState(1000 + cls)
  if cls == I64:
    i32 = np.iinfo(np.int32)
    v = [0, 1, -1, 2, -2, 3, -3, 7, -7, i32.min, i32.max, i32.max + 1, I64_MIN, I64_MIN + 1, I64_MAX]
    v += list(rng.randint(-10 ** 6, 10 ** 6, size=4)) + list(rng.randint(I64_MIN, I64_MAX, size=3, dtype=np.int64))
    return np.array(v, np.int64)
  dt = CLS_DT[cls]
  fi = np.finfo(dt)
  m = 24 if cls == F32 else 53
  nan_payload = np.array([0x7fc00123 if cls == F32 else 0x7ff8000000000123], np.uint32 if cls == F32 else
                         np.uint64).view(dt)[0]
  tiny_den = fi.smallest_subnormal
  big_den = fi.smallest_normal - fi.smallest_subnormal
  v = [0.0, -0.0, tiny_den, -tiny_den, big_den, fi.smallest_normal, 0.5, -0.5, 1, -1, 1.5, -1.5, 2.5, -2.5, 3, -3,
       2.0 ** m - 1, 2.0 ** m + 1, -(2.0 ** m + 1), fi.max, -fi.max, np.inf, -np.inf, np.nan, nan_payload]
  v += list(rng.randn(3) * 10) + list(rng.rand(2) * 1e-3)
  return np.array(v, dt)


def _coprime_len(n, V):
  while math.gcd(n, V * (V + 1)) != 1:
    n += 1
  return n


def _pad(arrs, n):
  return [np.concatenate([a, np.resize(a, n - len(a))]) for a in arrs]


def operand_rows(cls, arity):
  """The operands as equal-length 1-D arrays: the grid (unary), its Cartesian square (binary) or the (condition,
  value) square with a rotated third operand (WHERE), padded to a length coprime to V and V + 1."""
  g = edge_grid(cls)
  if arity == 1:
    ops = [g]
  else:
    a, b = np.meshgrid(g, g, indexing='ij')
    ops = [a.ravel(), b.ravel()]
    if arity == 3:
      ops.append(np.roll(ops[1], 7))
  n = _coprime_len(len(ops[0]), CLS_V[cls])
  return _pad(ops, n)


def bits_equal(got, want, what, inputs=()):
  got, want = np.asarray(got), np.asarray(want)
  assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
  assert got.shape == want.shape, (what, got.shape, want.shape)
  if got.dtype.kind == 'f':
    ib = np.dtype('u%d' % got.dtype.itemsize)
    same = (got.view(ib) == want.view(ib)) | (np.isnan(got) & np.isnan(want))
  else:
    same = got == want
  if not same.all():
    bad = np.argwhere(~same)[:8]
    rows = []
    for idx in bad:
      t = tuple(idx)
      rows.append('%s: in=%s got=%r want=%r' % (t, [x[t] if np.ndim(x) else x for x in inputs], got[t], want[t]))
    raise AssertionError('%s: %d of %d differ\n  %s' % (what, (~same).sum(), same.size, '\n  '.join(rows)))


def ulp_error(got, ref, dt):
  """|got - ref| in ulp of dt at ref; ref in a wider type.  Non-finite references must be met exactly."""
  got = np.asarray(got)
  wide = np.longdouble if dt == np.float64 else np.float64
  ref = np.asarray(ref, wide)
  err = np.zeros(got.shape, np.float64)
  fin = np.isfinite(ref)
  nf = ~fin
  ok_nf = (np.isnan(ref) & np.isnan(got)) | (ref == got.astype(wide))
  err[nf & ~ok_nf] = np.inf
  r = ref[fin]
  with np.errstate(all='ignore'):
    rr = r.astype(dt)                       # the correctly rounded result (inf past the largest finite value)
    sp = np.spacing(np.abs(rr)).astype(wide)
    sp = np.where(np.isfinite(sp) & (sp > 0), sp, np.spacing(np.finfo(dt).max))
    g = got[fin]
    e = np.abs(g.astype(wide) - r) / sp
  e[np.isnan(e)] = np.inf
  e[g == rr] = 0.0
  err[fin] = e.astype(np.float64)
  return err


# ------------------------------------------------------------------------------------------------- map launches
def _program(cls, op, n_in, shape, strides, in_dts, out_dt, const=None):
  """`op` on registers 0..n_in-1 into a fresh register, then MOV (so no program matches the prebuilt library and
  the interpreter / run-time specialised tiers are the ones that run)."""
  p = Program()
  for dt, st in zip(in_dts, strides):
    p.add_input(dt, st)
  r = n_in
  if op in ('ADDC', 'SUBC', 'RSUBC', 'MULC', 'DIVC', 'RDIVC', 'MAXC', 'MINC'):
    p.emit(op, r, p.add_const(const), 0)
  elif op == 'WHERE':
    p.emit(op, r, 0, 1, 2)
  elif n_in == 1:
    p.emit(op, r, 0)
  else:
    p.emit(op, r, 0, 1)
  p.emit('MOV', r + 1, r)
  p.result_reg = r + 1
  linear = all(tuple(st) == dense_strides(shape) or all(s == 0 for s in st) for st in strides)
  return p.finish(cls, shape, out_dt, linear)


def run_layout(cls, op, ops, layout, out_dt, const=None):
  """Launch `op` over operand rows `ops` in one of three layouts; returns (got, the operands as the output sees
  them)."""
  V = CLS_V[cls]
  n = len(ops[0])
  if layout == 'dense':
    # V + 1 copies: with n coprime to V every element meets every lane position of the vector body, plus a tail
    xs = [np.tile(a, V + 1) for a in ops]
    shape, strides, tens = (len(xs[0]),), [(1,)] * len(xs), [dev(x) for x in xs]
  elif layout == 'strided':
    # operand 0 a view with an odd element offset and a row pitch of W + 2: rows of W = V + 1 elements, the last one
    # evaluated by the scalar group of the ragged kernel; n coprime to W puts every element in every column
    W = V + 1
    xs = [np.tile(a, W).reshape(n, W) for a in ops]
    buf = np.zeros((n, W + 2), xs[0].dtype)
    buf[:, 1:W + 1] = xs[0]
    view = dev(buf)[:, 1:W + 1]
    shape = (n, W)
    strides = [(W + 2, 1)] + [(W, 1)] * (len(xs) - 1)
    tens = [view] + [dev(x) for x in xs[1:]]
  else:
    # operand 0 broadcast along the rows (inner stride 0), the others dense
    W = V + 1
    xs = [np.repeat(ops[0][:, None], W, 1)] + [np.tile(a, W).reshape(W, n).T.copy() for a in ops[1:]]
    shape = (n, W)
    strides = [(1, 0)] + [(W, 1)] * (len(xs) - 1)
    tens = [dev(ops[0].copy())] + [dev(x) for x in xs[1:]]
  prog = _program(cls, op, len(ops), shape, strides, [x.dtype for x in xs], out_dt, const)
  out = D.empty(shape, out_dt)
  kernels.map_fused(prog, tens, out)
  D.synchronize()
  return host(out), xs


def _consts(cls):
  g = edge_grid(cls)
  if cls == I64:
    return [int(c) for c in g[[0, 1, 2, 9, 12, 14]]]
  return [float(c) for c in g[[1, 2, 8, 9, 12, 21, 22, 23]]]


def reference(op, cls, xs, const=None):
  dt = CLS_DT[cls]
  spec = SEMANTICS[op]
  with np.errstate(all='ignore'):
    if spec['arity'] == 'c':
      return np.asarray(spec['ref'](xs[0], dt.type(const)))
    if op == 'POW' and cls == I64:
      return _np_int_pow(*xs)
    if spec['kind'] == 'ulp':
      wide = np.longdouble if cls == F64 else np.float64
      if op == 'NORM_CDF':
        return _norm_cdf(xs[0])
      return spec['ref'](*[x.astype(wide) for x in xs])
    return np.asarray(spec['ref'](*xs))


def out_dtype(op, cls, want):
  if SEMANTICS[op]['kind'] == 'ulp':
    return CLS_DT[cls]
  return want.dtype


def check_op(op, cls, got, xs, const=None, where=''):
  dt = CLS_DT[cls]
  want = reference(op, cls, xs, const)
  what = '%s %s %s' % (op, dt, where)
  if SEMANTICS[op]['kind'] == 'ulp' and not (op == 'POW' and cls == I64):
    err = ulp_error(got, want, dt)
    worst = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() <= ULP_BOUND, '%s: %.3g ulp at in=%s got=%r ref=%r' % (
        what, err.max(), [x[worst] for x in xs], got[worst], want[worst])
    _special_values(op, got, xs, what)
  else:
    bits_equal(got, want, what, xs)


def _special_values(op, got, xs, what):
  """The values the ulp bound does not speak for: exact."""
  x = xs[0]
  if op == 'EXP':
    for v, r in ((-np.inf, 0.0), (np.inf, np.inf), (0.0, 1.0)):
      assert np.all(got[x == v] == r), (what, v)
  elif op == 'LOG':
    assert np.all(got[x == 0] == -np.inf), what
    assert np.all(np.isnan(got[x < 0])) and np.all(got[x == 1] == 0), what
    assert np.all(got[x == np.inf] == np.inf), what
  elif op == 'TANH':
    assert np.all(got[x == np.inf] == 1) and np.all(got[x == -np.inf] == -1), what
  elif op == 'POW':
    assert np.all(got[xs[1] == 0] == 1), what                  # x ** 0 == 1, NaN included
    assert np.all(got[(x == 1) & ~np.isnan(xs[1])] == 1), what
  elif op == 'NORM_CDF':
    assert np.all(got[x == np.inf] == 1) and np.all(got[x == -np.inf] == 0), what
  assert np.all(np.isnan(got[np.isnan(x) & ~((op == 'POW') & (xs[-1] == 0))])), what


def _cases():
  out = []
  for op, spec in SEMANTICS.items():
    if spec['ref'] is None:
      continue
    for cls in spec['classes']:
      out.append(pytest.param(op, cls, id='%s-%s' % (op, CLS_DT[cls].name)))
  return out


def _arity(op):
  a = SEMANTICS[op]['arity']
  return 1 if a == 'c' else a


def _run_all_layouts(op, cls, layouts):
  """[(layout, const, got, xs)] for every layout (and constant of a *C opcode)."""
  ops = operand_rows(cls, _arity(op))
  consts = _consts(cls) if SEMANTICS[op]['arity'] == 'c' else [None]
  res = []
  for const in consts:
    want = reference(op, cls, [o for o in ops], const)
    odt = out_dtype(op, cls, np.asarray(want))
    for layout in layouts:
      got, xs = run_layout(cls, op, ops, layout, odt, const)
      res.append((layout, const, got, xs))
  return res


@pytest.mark.gpu
@pytest.mark.parametrize('op,cls', _cases())
def test_opcode_interpreter(op, cls):
  """Interpreter tier, three layouts: dense (every element at every lane of the V-wide body, and in the tail), one
  operand broadcast (stride 0), one operand a strided view with an odd offset (the ragged kernel's scalar group)."""
  with _interpreted():
    for layout, const, got, xs in _run_all_layouts(op, cls, ('dense', 'broadcast', 'strided')):
      check_op(op, cls, got, xs, const, '%s const=%r' % (layout, const))


@pytest.mark.gpu
@pytest.mark.parametrize('op,cls', _cases())
def test_opcode_jit_tier_is_the_interpreter(op, cls):
  """The hipRTC-built kernel of the same program: bit-identical to the interpreter (transcendentals included) and to
  NumPy within the same contract.  Dense layout only: the compile cache is keyed on the program."""
  before = _hip.lib().sp_jit_compiled_count()
  want, got, got2 = _both_tiers(lambda: _run_all_layouts(op, cls, ('dense',)))
  # (every (opcode, class) is a program of its own: its specialisation is new, so the count must move)
  assert _hip.lib().sp_jit_compiled_count() > before, 'program was not specialised at run time'
  for (_, const, w, xs), (_, _, g, _), (_, _, g2, _) in zip(want, got, got2):
    bits_equal(g, w, '%s %s jit vs interpreter const=%r' % (op, CLS_DT[cls], const), xs)
    bits_equal(g2, w, '%s %s jit (cached) const=%r' % (op, CLS_DT[cls], const), xs)
    check_op(op, cls, g, xs, const, 'jit const=%r' % (const,))


@pytest.mark.gpu
@pytest.mark.parametrize('cls', ALL)
def test_const_and_iota(cls):
  dt = CLS_DT[cls]
  for c in _consts(cls):
    p = Program()
    p.emit('CONST', 0, p.add_const(c))
    p.emit('IOTA', 1)
    p.emit('ADD', 2, 0, 1)
    p.emit('NOP', 3)
    p.result_reg = 2
    shape = (37, 5)
    prog = p.finish(cls, shape, dt, True)
    out = D.empty(shape, dt)
    with _interpreted():
      kernels.map_fused(prog, [], out)
    D.synchronize()
    with np.errstate(all='ignore'):
      want = (dt.type(c) + np.arange(37 * 5).astype(dt)).reshape(shape)
    bits_equal(host(out), want, 'CONST %r + IOTA %s' % (c, dt))


@pytest.mark.gpu
@pytest.mark.parametrize('cls', ALL)
def test_store_casts_are_astype(cls):
  """The class value stored into each output dtype (sp_store_vec) is ndarray.astype of it: for floats, NaN / inf /
  out-of-range give INT_MIN of the width (uint8 through int32), as x86 NumPy does."""
  ops = operand_rows(cls, 1)
  extra = np.array([3e9, -3e9, 300.0, 255.9, -1.0, -0.9, 2147483520.0, 1e20], np.float64)
  if cls != I64:
    ops = _pad([np.concatenate([ops[0], extra.astype(CLS_DT[cls])])], _coprime_len(len(ops[0]) + 8, CLS_V[cls]))
  for odt in (np.float32, np.float64, np.int32, np.int64, np.bool_, np.uint8):
    for layout in ('dense', 'strided'):
      with _interpreted():
        got, xs = run_layout(cls, 'MOV', ops, layout, odt)
      with np.errstate(all='ignore'):
        want = xs[0].astype(odt)
      bits_equal(got, want, 'store %s -> %s %s' % (CLS_DT[cls], np.dtype(odt), layout), xs)


@pytest.mark.gpu
@pytest.mark.parametrize('sid,name', [(1, 'ADDC'), (2, 'SUBC'), (3, 'MULC'), (4, 'DIVC'), (5, 'ADD'), (6, 'SUB'),
                                      (7, 'MUL'), (8, 'DIV'), (9, 'x*x+x'), (10, 'x*(yp-y)'), (11, 'x*x'),
                                      (12, 'RSUBC')])
def test_prebuilt_programs(sid, name):
  """The twelve prebuilt fp32 programs (sp_interp.hpp StaticProg 1-12) over the fp32 grid, dense and strided."""
  import ctypes as C
  ops = operand_rows(F32, 2)
  consts = _consts(F32) if name.endswith('C') else [None]
  for const in consts:
    for layout in ('dense', 'strided'):
      V = 4
      n = len(ops[0])
      nin = {9: 1, 11: 1, 10: 3}.get(sid, 1 if name.endswith('C') else 2)
      src = (ops + [np.roll(ops[1], 3)])[:nin]
      if layout == 'dense':
        xs = [np.tile(a, V + 1) for a in src]
        shape, strides, tens = (len(xs[0]),), [(1,)] * nin, [dev(x) for x in xs]
      else:
        W = 2 * V      # rows a multiple of V: the prebuilt kernel's own strided (2-D) path
        xs = [np.tile(a, W).reshape(n, W) for a in src]
        buf = np.zeros((n, W + 2), np.float32)
        buf[:, 1:W + 1] = xs[0]
        shape, strides = (n, W), [(W + 2, 1)] + [(W, 1)] * (nin - 1)
        tens = [dev(buf)[:, 1:W + 1]] + [dev(x) for x in xs[1:]]
      p = Program()
      for st in strides:
        p.add_input(np.float32, st)
      if name.endswith('C'):
        p.emit(name, 1, p.add_const(const), 0)
        p.result_reg = 1
      elif sid in (5, 6, 7, 8):
        p.emit(name, 2, 0, 1)
        p.result_reg = 2
      elif sid == 9:
        p.emit('MUL', 1, 0, 0)
        p.emit('ADD', 1, 1, 0)
        p.result_reg = 1
      elif sid == 10:
        p.emit('SUB', 3, 1, 2)
        p.emit('MUL', 3, 0, 3)
        p.result_reg = 3
      else:
        p.emit('MUL', 1, 0, 0)
        p.result_reg = 1
      linear = layout == 'dense'
      prog = p.finish(F32, shape, np.float32, linear)
      assert _hip.lib().sp_program_static_id(C.byref(prog), F32) == sid
      out = D.empty(shape, np.float32)
      kernels.map_fused(prog, tens, out)
      D.synchronize()
      c = np.float32(const) if const is not None else None
      x = xs[0]
      with np.errstate(all='ignore'):
        want = {1: lambda: x + c, 2: lambda: x - c, 3: lambda: x * c, 4: lambda: x / c, 5: lambda: x + xs[1],
                6: lambda: x - xs[1], 7: lambda: x * xs[1], 8: lambda: x / xs[1], 9: lambda: x * x + x,
                10: lambda: x * (xs[1] - xs[2]), 11: lambda: x * x, 12: lambda: c - x}[sid]()
      bits_equal(host(out), want, 'static %d (%s) %s const=%r' % (sid, name, layout, const), xs)


# ------------------------------------------------------------------------------------------------- reductions
# shapes from sp_plan (reduce_impl.hpp), for V = 4 (fp32) and V = 2 (fp64 / int64); (shape, axis, plan)
RED_SHAPES = [
    ((1024, 37), 1, 'rows-wave: I = 1, A <= 64 V 16, O >= 1024'),
    ((3, 40000), 1, 'rows split across workgroups (A > 8 * 256 V), sp_finish_rows_kernel'),
    ((5, 1001), 1, 'single row pass: A below one split chunk, O < 1024'),
    ((1000, 8), 0, 'columns split (A / 64 chunks), sp_finish_cols_kernel'),
    ((1000, 9), 0, 'column tail kernel: I % V != 0, also split'),
    ((3, 40000), None, 'axis=None: one row of 120000, split'),
]


def _plant_positions(A):
  return {'first': 0, 'last': A - 1, 'other-chunk': A // 2 + 1}


def _red_base(cls, op, shape, rng):
  dt = CLS_DT[cls]
  if op == 'PROD':
    x = np.ones(shape)
    x[rng.rand(*shape) < 0.01] = -1
  elif op in ('AND',):
    x = rng.randint(1, 4, size=shape)
  elif op == 'OR':
    x = (rng.rand(*shape) < 0.001).astype(np.int64)
  else:
    x = rng.randint(-8, 9, size=shape)          # integer-valued: every partial sum is exact, so sums are bit-exact
  return x.astype(dt)


def _red_scenarios(cls, op):
  """name -> (values planted at (position, other position)) for the reduced axis."""
  if cls == I64:
    s = {'int64-min': (I64_MIN, I64_MIN), 'int64-max': (I64_MAX, I64_MAX)}
    if op in ('AND', 'OR'):
      s['zero'] = (0, 0)
    return s
  s = {'nan': (np.nan, None), 'inf-and-minus-inf': (np.inf, -np.inf), 'minus-zero': (-0.0, None),
       'plus-zero': (0.0, None), 'all-minus-inf': (-np.inf, None), 'all-plus-inf': (np.inf, None)}
  return s


def _red_ref(op, v, axis, dt):
  with np.errstate(all='ignore'):
    r = REDUCTIONS[op](v, axis=axis)
  if op in ('AND', 'OR'):
    return np.asarray(r, np.bool_)
  return np.asarray(r, dt)


def _run_red_cases(cls, op, shape, axis):
  dt = CLS_DT[cls]
  rng = np.random.RandomState(7)
  base = _red_base(cls, op, shape, rng)
  A = base.size if axis is None else shape[axis]
  odt = np.bool_ if op in ('AND', 'OR') else dt
  results = []
  for name, (v0, v1) in sorted(_red_scenarios(cls, op).items()):
    for pname, pos in sorted(_plant_positions(A).items()):
      x = base.copy()
      xv = x.reshape(-1) if axis is None else np.moveaxis(x, axis, -1)
      xv[..., pos] = v0
      if v1 is not None:
        xv[..., (pos + A // 2) % A] = v1          # the other value in another chunk of the same row
      if name in ('minus-zero', 'plus-zero') or name.startswith(('int64', 'all-')):
        xv[...] = v0                              # whole rows of the value: the identity must not leak into them
      got = run_reduce(x, axis, op, cls, odt, body=_mov_body)
      results.append(('%s@%s' % (name, pname), x, got))
  return results


def _mov_body(p):
  p.emit('MOV', 1, 0)     # outside the prebuilt library: the interpreter / run-time specialised kernels
  return 1


@pytest.mark.gpu
@pytest.mark.parametrize('cls', ALL, ids=lambda c: CLS_DT[c].name)
@pytest.mark.parametrize('op', list(REDUCTIONS))
@pytest.mark.parametrize('shape,axis,plan', RED_SHAPES, ids=[s[2].split(':')[0] for s in RED_SHAPES])
def test_reducer_edges_both_tiers(cls, op, shape, axis, plan):
  want, got, got2 = _both_tiers(lambda: _run_red_cases(cls, op, shape, axis))
  for (case, x, w), (_, _, g), (_, _, g2) in zip(want, got, got2):
    what = '%s %s %s %s [%s]' % (op, CLS_DT[cls], case, plan, shape)
    bits_equal(g, w, what + ' jit vs interpreter')
    bits_equal(g2, w, what + ' jit cached')
    ref = _red_ref(op, x, axis, CLS_DT[cls])
    bits_equal(np.asarray(w), ref, what)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [np.int32, np.bool_, np.uint8])
def test_narrow_integer_sums_widen_to_int64(dt):
  """int32 / bool / uint8 tiles summed in the int64 class: NumPy's int64 result (no int32 wrap)."""
  rng = np.random.RandomState(3)
  if dt == np.int32:
    x = np.full((5, 3001), np.iinfo(np.int32).max, np.int32)
    x[:, ::7] = np.iinfo(np.int32).min
  elif dt == np.bool_:
    x = rng.rand(5, 3001) < 0.7
  else:
    x = rng.randint(200, 256, size=(5, 3001)).astype(np.uint8)
  for axis in (None, 0, 1):
    got = run_reduce(x, axis, 'SUM', I64, np.int64)
    bits_equal(np.asarray(got), np.asarray(x.sum(axis, dtype=np.int64)), 'sum %s axis=%s' % (np.dtype(dt), axis))


# ------------------------------------------------------------------------------------------------- arg-reductions
def _run_arg(x, axis, which, cls, sentinel=-7):
  shape = x.shape
  O = int(np.prod(shape[:axis], dtype=np.int64))
  A = shape[axis]
  I = int(np.prod(shape[axis + 1:], dtype=np.int64))
  p = Program()
  p.add_input(x.dtype, dense_strides((O, A, I)))
  p.emit('MOV', 1, 0)
  p.result_reg = 1
  prog = p.finish(cls, (O, A, I), None, True)
  oi = D.empty((O * I,), np.int64)
  ov = D.empty((O * I,), CLS_DT[cls])
  kernels.argreduce(prog, [dev(x)], which, O, A, I, 0, sentinel, oi, ov)
  D.synchronize()
  rs = shape[:axis] + shape[axis + 1:]
  return host(oi).reshape(rs), host(ov).reshape(rs)


def _arg_rows(cls, A):
  """Rows of the arg-reduction edge cases, each with its NumPy answers."""
  dt = CLS_DT[cls]
  rng = np.random.RandomState(11)
  rows = []
  if cls == I64:
    for v in (I64_MIN, I64_MAX):
      r = rng.randint(-5, 5, size=A).astype(np.int64)
      r[[3, A // 2 + 1, A - 1]] = v                # ties of an extreme: the first one wins
      rows.append(r)
    rows.append(np.full(A, I64_MIN, np.int64))
    rows.append(np.full(A, I64_MAX, np.int64))
    return rows
  r = np.full(A, np.inf, dt)
  rows.append(r)
  rows.append(-r)
  r = rng.randint(-5, 5, size=A).astype(dt)
  r[[2, A - 2]] = np.inf
  r[[5, A - 1]] = -np.inf
  rows.append(r)
  rows.append(np.full(A, np.nan, dt))              # all NaN: the sentinel
  r = rng.randint(-5, 5, size=A).astype(dt)
  r[[1, 4]] = 9
  r[6] = np.nan                                   # a NaN after a tie: the sentinel
  rows.append(r)
  r = rng.randint(-5, 5, size=A).astype(dt)
  r[[A // 3, A // 2 + 1, A - 1]] = 50              # a tie across split chunks: the first occurrence wins
  r[[A // 4, A - 3]] = -50
  rows.append(r)
  r = np.zeros(A, dt)
  r[::2] = -0.0                                    # +-0 ties: equal, first occurrence
  rows.append(r)
  return rows


@pytest.mark.gpu
@pytest.mark.parametrize('cls', ALL, ids=lambda c: CLS_DT[c].name)
@pytest.mark.parametrize('A,axis', [(37, 1), (40000, 1), (1000, 0), (1001, 0)])
def test_argreduce_edges_both_tiers(cls, A, axis):
  rows = np.stack(_arg_rows(cls, A))             # [R, A]
  x = rows if axis == 1 else np.ascontiguousarray(rows.T)

  def run():
    return [_run_arg(x, axis, which, cls) for which in (0, 1)]
  want, got, got2 = _both_tiers(run)
  for which in (0, 1):
    bits_equal(got[which][0], want[which][0], 'arg%s jit' % which)
    bits_equal(got2[which][0], want[which][0], 'arg%s jit cached' % which)
    bits_equal(got[which][1], want[which][1], 'arg%s jit value' % which)
    bits_equal(got2[which][1], want[which][1], 'arg%s jit cached value' % which)
    idx, val = want[which]
    for k, r in enumerate(rows):
      if cls != I64 and np.isnan(r).any():
        assert idx[k] == -7 and np.isnan(val[k]), (which, k, idx[k])
        continue
      ref = np.argmax(r) if which == 0 else np.argmin(r)
      assert idx[k] == ref, ('arg%s' % ['max', 'min'][which], CLS_DT[cls], A, k, idx[k], ref)
      bits_equal(np.asarray(val[k]), np.asarray(r[ref]), 'arg value row %d' % k)


# ------------------------------------------------------------------------------------------------- merge kernel
UPD_DTYPES = [np.float32, np.float64, np.int32, np.int64, np.bool_, np.uint8]


def _upd_values(dt, n, rng):
  dt = np.dtype(dt)
  if dt.kind == 'f':
    v = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3.0, 2.5, 300.0, 3e9, -3e9], np.float64)
    return rng.permutation(np.resize(v, n)).astype(dt)
  if dt == np.bool_:
    return rng.rand(n) < 0.5
  info = np.iinfo(dt)
  v = np.array([0, 1, -1, 2, 7, 255, 256, 300, info.max, info.min, info.max - 1], np.int64)
  if dt == np.int64:
    v = np.concatenate([v, [2 ** 32 + 1, -2 ** 33, 3000000000]])
  return np.resize(v, n).astype(dt)


@pytest.mark.gpu
@pytest.mark.parametrize('dst', UPD_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('reducer', list(MERGE_REDUCERS))
def test_update_reducers_dtypes_masks(dst, reducer):
  """Tile.merge (tile.pyx:250-283): dst[box] = reducer(dst[box], upd) -- computed in NumPy's promoted dtype, then
  cast to dst.dtype -- where the mask says the cell was written, upd.astype(dst.dtype) where not; updates of every
  dtype, with values the tile's dtype cannot hold (NaN, 3e9, 300, -1, integer extremes); boxes whose inner extent is
  (6 x 8) and is not (5 x 7) a multiple of V.  Among them: NaN under MAX / MIN, int32 / uint8 wrap-around under
  ADD / MUL, bool ADD as logical or."""
  rng = np.random.RandomState(5)
  for src in UPD_DTYPES:
    for box in (((1, 0), (7, 8)), ((2, 1), (7, 8))):
      (r0, c0), (r1, c1) = box
      bshape = (r1 - r0, c1 - c0)
      old = _upd_values(dst, 9 * 8, rng).reshape(9, 8)
      upd = _upd_values(src, bshape[0] * bshape[1], np.random.RandomState(6)).reshape(bshape)
      maskv = rng.rand(9, 8) < 0.5
      with np.errstate(all='ignore'):
        u = upd.astype(dst)
      for mode in (_hip.MASK_ALL_CLEAR, _hip.MASK_ALL_SET, _hip.MASK_ARRAY):
        t = dev(old.copy())
        m = dev(maskv.astype(np.uint8)) if mode == _hip.MASK_ARRAY else None
        kernels.update(t, (r0, c0), (r1, c1), dev(upd), reducer, mode, m)
        D.synchronize()
        want = old.copy()
        region = want[r0:r1, c0:c1]
        fn = MERGE_REDUCERS[reducer]
        written = {_hip.MASK_ALL_CLEAR: np.zeros(bshape, bool), _hip.MASK_ALL_SET: np.ones(bshape, bool),
                   _hip.MASK_ARRAY: maskv[r0:r1, c0:c1]}[mode]
        with np.errstate(all='ignore'):
          merged = u if fn is None else np.asarray(fn(region, upd)).astype(dst)
        region[...] = np.where(written, merged, u)
        what = 'update %s <- %s %s mode=%d box=%s' % (np.dtype(dst), np.dtype(src), reducer, mode, box)
        bits_equal(host(t), want, what, (np.pad(u, ((r0, 9 - r1), (c0, 8 - c1))), old))
        if m is not None:
          wm = maskv.astype(np.uint8)
          wm[r0:r1, c0:c1] = 1
          bits_equal(host(m), wm, what + ' mask')


@pytest.mark.gpu
@pytest.mark.parametrize('dst,old,src,upd,reducer,want', [
    (np.uint8, 200, np.int64, 300, 'MAX', 44),        # max(200, 300) = 300 -> 44, not max(200, 44)
    (np.bool_, True, np.int64, -1, 'ADD', False),     # True + -1 = 0
    (np.bool_, True, np.uint8, 255, 'ADD', False),    # uint8: 1 + 255 wraps to 0
    (np.bool_, True, np.int32, -1, 'MUL', True),
    (np.int32, 3, np.float64, -0.5, 'ADD', 2),        # 2.5 -> 2, not 3 + int(-0.5) = 3
    (np.uint8, 200, np.float32, 100.5, 'ADD', 44),    # float32 300.5 -> 300 -> 44
    (np.int32, 1, np.float64, 3e9, 'NONE', np.iinfo(np.int32).min),
    (np.float32, 1.0, np.float64, 2.0 ** -30, 'ADD', 1.0),
])
def test_update_reduces_before_it_casts(dst, old, src, upd, reducer, want):
  """The reference's rule (tile.pyx:263-279): reduce in NumPy's promoted dtype, then cast to the tile's dtype."""
  t = dev(np.full((2, 5), old, dst))
  kernels.update(t, (0, 0), (2, 5), dev(np.full((2, 5), upd, src)), reducer, _hip.MASK_ALL_SET, None)
  D.synchronize()
  with np.errstate(all='ignore'):
    ref = np.asarray(MERGE_REDUCERS[reducer](np.full((2, 5), old, dst), np.full((2, 5), upd, src))
                     if reducer != 'NONE' else np.full((2, 5), upd, src)).astype(dst)
  bits_equal(ref, np.full((2, 5), want, dst), 'NumPy itself')
  bits_equal(host(t), ref, '%s %r %s %s %r' % (np.dtype(dst), old, reducer, np.dtype(src), upd))


@pytest.mark.gpu
@pytest.mark.parametrize('fdt', [np.float32, np.float64])
def test_float_operand_of_the_int64_class_is_astype(fdt):
  """A float operand loaded into the int64 class (sp_load_vec -> sp_cvt) converts as ndarray.astype(int64) does."""
  x = edge_grid(F32 if fdt == np.float32 else F64).astype(fdt)
  x = _pad([np.concatenate([x, np.array([3e9, -3e9, 9.2e18, 9.3e18, -9.3e18, 255.9, -0.9], fdt)])],
           _coprime_len(len(x) + 7, 2))[0]
  for layout in ('dense', 'strided'):
    with _interpreted():
      got, xs = run_layout(I64, 'MOV', [x], layout, np.int64)
    with np.errstate(all='ignore'):
      bits_equal(got, xs[0].astype(np.int64), 'int64 class <- %s %s' % (np.dtype(fdt), layout), xs)


# ------------------------------------------------------------------------------------------------- public lowering
# The same edges through HipBackend._run_map: the class choice (lower.choose_class) and the TO_* normalisation of the
# Emitter (lower.py), not just the kernels.
def _cast_values(dt):
  f = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 0.5, -0.9, 1.5, -2.5, 255.9, 300.0, -1.0, 3e9, -3e9,
                2147483520.0, 1e20, 9.2e18, 9.3e18, 5e-324, 1e-40, np.finfo(np.float64).max], np.float64)
  i = np.array([0, 1, -1, 255, 256, 300, -129, 2 ** 31 - 1, 2 ** 31, -2 ** 31, I64_MIN, I64_MAX, 2 ** 53 + 1,
                16777217, 7], np.int64)
  dt = np.dtype(dt)
  with np.errstate(all='ignore'):
    if dt == np.bool_:
      v = np.array([True, False, True], np.bool_)
    elif dt.kind == 'f':
      v = f.astype(dt)
    else:
      v = i.astype(dt)
  return np.resize(v, 37)       # an odd length: a scalar tail behind the vector body


_BE = []


def _lowered(root):
  from spartan_amd.backend_hip import HipBackend
  if not _BE:
    _BE.append(HipBackend())
  return host(_BE[0]._run_map(root, root.shape))


def _T(a):
  from spartan_amd import lower
  return lower.V('tensor', dtype=a.dtype, shape=a.shape, tensor=dev(a))


def _ap(name, fn, *args):
  from spartan_amd import lower
  return lower.apply(name, fn, list(args))


@pytest.mark.gpu
@pytest.mark.parametrize('src', UPD_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('dst', UPD_DTYPES, ids=lambda d: np.dtype(d).name)
def test_astype_through_the_lowering(src, dst):
  from spartan_amd import lower
  x = _cast_values(src)
  root = lower.cast(_T(x), dst)
  if root.kind == 'tensor':
    root = _ap('MAX', np.maximum, root, _T(x))     # (a no-op cast lowers to nothing: give it a program)
  with np.errstate(all='ignore'):
    want = x.astype(dst)
  bits_equal(_lowered(root), want, 'astype %s -> %s' % (np.dtype(src), np.dtype(dst)), (x,))


@pytest.mark.gpu
def test_narrow_integer_chains_wrap_like_numpy():
  """int32 (a * b) // c and (a - b) % c with a * b past 2^31, uint8 a - b below 0: each intermediate wraps in its
  own dtype (the int64 class re-normalises it with TO_I32 / TO_U8)."""
  rng = np.random.RandomState(21)
  a = np.concatenate([[70000, -70000, 46341, 2 ** 31 - 1, -2 ** 31, -2 ** 31, 3], rng.randint(-10 ** 5, 10 ** 5, 30)])
  b = np.concatenate([[70000, 3, 46341, 2, 1, 2, -1], rng.randint(-10 ** 5, 10 ** 5, 30)])
  c = np.concatenate([[7, -7, 3, 1, -1, 5, 2], rng.randint(1, 50, 30) * rng.choice([-1, 1], 30)])
  a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
  A, B, C = _T(a), _T(b), _T(c)
  with np.errstate(all='ignore'):
    cases = [
        ('(a*b)//c', _ap('FLOORDIV', np.floor_divide, _ap('MUL', np.multiply, A, B), C), (a * b) // c),
        ('(a-b)%c', _ap('MOD', np.mod, _ap('SUB', np.subtract, A, B), C), (a - b) % c),
        ('(a*b)%c', _ap('MOD', np.mod, _ap('MUL', np.multiply, A, B), C), (a * b) % c),
    ]
  u = rng.randint(0, 256, 37).astype(np.uint8)
  v = rng.randint(0, 256, 37).astype(np.uint8)
  w = rng.randint(1, 256, 37).astype(np.uint8)
  U, Vv, W = _T(u), _T(v), _T(w)
  with np.errstate(all='ignore'):
    cases += [
        ('u8 a-b', _ap('SUB', np.subtract, U, Vv), u - v),
        ('u8 (a-b)//c', _ap('FLOORDIV', np.floor_divide, _ap('SUB', np.subtract, U, Vv), W), (u - v) // w),
        ('u8 (a*b)%c', _ap('MOD', np.mod, _ap('MUL', np.multiply, U, Vv), W), (u * v) % w),
    ]
  for what, root, want in cases:
    bits_equal(_lowered(root), want, what)


@pytest.mark.gpu
def test_mixed_classes_through_the_lowering():
  """float32 (.) int64 computes in the float64 class; bool (.) bool under + / * is logical or / and."""
  x = edge_grid(F32)[:, None].copy()                 # (G, 1) against (1, H): every pair
  k = edge_grid(I64)[None, :].copy()
  X, K = _T(x), _T(k)
  for name, fn in (('ADD', np.add), ('SUB', np.subtract), ('MUL', np.multiply), ('DIV', np.divide),
                   ('MAX', np.maximum), ('MIN', np.minimum), ('FLOORDIV', np.floor_divide), ('MOD', np.mod),
                   ('LT', np.less), ('EQ', np.equal)):
    with np.errstate(all='ignore'):
      want = fn(x, k)
    bits_equal(_lowered(_ap(name, fn, X, K)), want, 'f32 %s i64' % name, (np.broadcast_to(x, want.shape),
                                                                          np.broadcast_to(k, want.shape)))
  p = np.array([True, False, True, False] * 9 + [True])
  q = np.array([True, True, False, False] * 9 + [False])
  P, Q = _T(p), _T(q)
  bits_equal(_lowered(_ap('ADD', np.add, P, Q)), p + q, 'bool + bool')
  bits_equal(_lowered(_ap('MUL', np.multiply, P, Q)), p * q, 'bool * bool')


@pytest.mark.gpu
@pytest.mark.parametrize('op', ['EXP', 'LOG', 'TANH', 'SQRT', 'POW'])
def test_float32_transcendentals_inside_the_float64_class(op):
  """f(x32) + int64 zeros: f is evaluated in the float64 class and rounded ONCE to float32 (TO_F32) -- within
  ULP_BOUND of the exact value and of NumPy's own float32 result."""
  fn = {'EXP': np.exp, 'LOG': np.log, 'TANH': np.tanh, 'SQRT': np.sqrt, 'POW': np.power}[op]
  g = edge_grid(F32)
  if op == 'POW':
    a, b = np.meshgrid(g, g, indexing='ij')
    args = [a.ravel().copy(), b.ravel().copy()]
  else:
    args = [g]
  z = np.zeros(args[0].shape, np.int64)
  root = _ap('ADD', np.add, _ap(op, fn, *[_T(a) for a in args]), _T(z))
  got = _lowered(root)
  with np.errstate(all='ignore'):
    want32 = fn(*args) + z                            # NumPy: float32 f, then float64
    exact = fn(*[a.astype(np.float64) for a in args])
  assert got.dtype == want32.dtype == np.float64
  bits_equal(got.astype(np.float32).astype(np.float64), got, '%s rounded once to float32' % op)
  err = ulp_error(got.astype(np.float32), exact, np.float32)
  assert err.max() <= ULP_BOUND, (op, err.max(), [a[np.argmax(err)] for a in args])
  err = ulp_error(got.astype(np.float32), want32, np.float32)
  assert err.max() <= ULP_BOUND, (op, 'vs NumPy float32', err.max(), [a[np.argmax(err)] for a in args])


@pytest.mark.gpu
def test_int32_overflow_inside_a_float_class_is_a_cast():
  """Documented deviation (DESIGN.md section c): an int32 product past 2^31 in an expression with a float operand is
  re-normalised by TO_I32 in the float64 class -- INT32_MIN, where NumPy wraps it in int32 arithmetic."""
  a = np.array([70000, 3, -70000, 46341, 100], np.int32)
  b = np.array([70000, 5, 70000, 46341, -7], np.int32)
  x = np.array([0.5, 0.25, -1.5, 2.0, 1.0], np.float32)
  got = _lowered(_ap('ADD', np.add, _ap('MUL', np.multiply, _T(a), _T(b)), _T(x)))
  with np.errstate(all='ignore'):
    numpy = (a * b) + x
  over = np.abs(a.astype(np.int64) * b) >= 2 ** 31
  assert over.sum() == 3
  bits_equal(got[~over], numpy[~over], 'in range: NumPy')
  bits_equal(got[over], np.iinfo(np.int32).min + x[over].astype(np.float64), 'past 2^31: INT32_MIN')


@pytest.mark.gpu
def test_reciprocal_of_an_int32_zero():
  """Documented deviation (DESIGN.md section c): np.reciprocal of an int32 0 is 0 here (the int64 class's INT64_MIN,
  wrapped to int32), INT32_MIN in NumPy; every other value, and the int64 0, as NumPy."""
  x = np.array([0, 1, -1, 2, -2, 7, np.iinfo(np.int32).min, np.iinfo(np.int32).max], np.int32)
  got = _lowered(_ap('RECIP', np.reciprocal, _T(x)))
  with np.errstate(all='ignore'):
    want = np.reciprocal(x)
  assert want[0] == np.iinfo(np.int32).min and got.dtype == np.int32
  assert got[0] == 0
  bits_equal(got[1:], want[1:], 'reciprocal int32')
  x64 = x.astype(np.int64)
  with np.errstate(all='ignore'):
    bits_equal(_lowered(_ap('RECIP', np.reciprocal, _T(x64))), np.reciprocal(x64), 'reciprocal int64')
