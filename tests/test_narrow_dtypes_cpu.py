"""The narrow element types (int8, int16, uint16, uint32, float16) on the host side: codes, arithmetic classes, result
dtypes of lowered trees and the narrowing steps of their instruction streams.  No GPU."""
import itertools

import numpy as np
import pytest

from spartan_amd import _hip, lower
from spartan_amd.program import class_of

ALL = [np.dtype(t) for t in (np.float32, np.float64, np.int32, np.int64, np.bool_, np.uint8,
                             np.int8, np.int16, np.uint16, np.uint32, np.float16)]
NEW = ALL[6:]


def test_dtype_code_round_trip():
  assert [_hip.sp_dtype(t) for t in ALL] == list(range(11))          # the first six keep their codes
  for t in ALL:
    assert _hip.np_dtype(_hip.sp_dtype(t)) == t
  assert (_hip.SP_I8, _hip.SP_I16, _hip.SP_U16, _hip.SP_U32, _hip.SP_F16) == (6, 7, 8, 9, 10)


def test_header_and_binding_agree_on_the_codes():
  import os
  import re
  text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'spartan_hip.h')).read()
  body = text.split('enum sp_dtype {')[1].split('}')[0]
  codes = {m.group(1): int(m.group(2)) for m in re.finditer(r'SP_(\w+) = (\d+)', body)}
  assert codes == {'F32': 0, 'F64': 1, 'I32': 2, 'I64': 3, 'BOOL': 4, 'U8': 5, 'I8': 6, 'I16': 7, 'U16': 8, 'U32': 9,
                   'F16': 10, 'DTYPE_COUNT': 11}
  assert '#define SP_ABI_VERSION 1' in text


def test_class_of_the_new_types():
  assert class_of(np.float16) == _hip.SP_F32                           # every half is a float
  for t in (np.int8, np.int16, np.uint16, np.uint32):
    assert class_of(t) == _hip.SP_I64


@pytest.mark.parametrize('bad', [np.uint64, np.complex64])
def test_types_that_stay_refused(bad):
  with pytest.raises(TypeError) as e:
    _hip.sp_dtype(bad)
  msg = str(e.value)
  assert msg.startswith('dtype %s is not supported by the HIP tile backend (supported: ' % np.dtype(bad))
  listed = msg.split('(supported: ')[1].rstrip(')').split()
  assert sorted(listed) == sorted(str(t) for t in ALL)


def test_opcode_names_are_unchanged():
  # 50 names: the narrowing of the new types is a width selector on TO_F32 / TO_I32 / TO_U8, not a new opcode
  assert len(_hip.OP) == 50
  assert {k for k in _hip.OP if k.startswith('TO_')} == {'TO_F32', 'TO_I32', 'TO_I64', 'TO_BOOL', 'TO_U8'}
  assert len(_hip.RED) == 6 and len(_hip.REDUCER) == 7


def _tensor(dt, shape=(4, 6)):
  return lower.V('tensor', dtype=dt, shape=shape, tensor=np.zeros(shape, dt))


@pytest.mark.parametrize('a,b', list(itertools.product(ALL, ALL)), ids=lambda t: str(t))
def test_result_dtype_is_numpys_for_every_pair(a, b):
  for name, fn in (('ADD', np.add), ('MUL', np.multiply)):
    got = lower.apply(name, fn, [_tensor(a), _tensor(b)]).dtype
    assert got == np.result_type(a, b), (name, a, b, got)


def test_promotions_the_kernels_rely_on():
  r = np.result_type
  assert r(np.int8, np.uint8) == np.int16 and r(np.uint16, np.int16) == np.int32 and r(np.uint32, np.int32) == np.int64
  assert r(np.float16, np.int16) == np.float32 and r(np.float16, np.int32) == np.float64
  assert r(np.float16, np.int8) == np.float16 and r(np.float32, np.uint32) == np.float64


@pytest.mark.parametrize('dt', NEW, ids=lambda t: str(t))
def test_weak_python_scalars_keep_the_narrow_type(dt):
  one = 1.0 if dt.kind == 'f' else 1
  v = lower.apply('ADD', np.add, [_tensor(dt), lower.const(one)])
  assert v.dtype == dt


def _stream(root, out_dtype):
  from spartan_amd.program import class_of as cls_of
  cls = lower.choose_class(root, [cls_of(out_dtype)])
  prog, _ = lower.Emitter(cls, root.shape).finish(root, out_dtype)
  names = {v: k for k, v in _hip.OP.items()}
  return prog, [(names[prog.instr[i].op], prog.instr[i].c) for i in range(prog.n_instr)]


@pytest.mark.parametrize('dt,narrow', [(np.int8, ('TO_I32', 1)), (np.int16, ('TO_I32', 2)), (np.uint16, ('TO_U8', 1)),
                                       (np.uint32, ('TO_U8', 2)), (np.float16, ('TO_F32', 1))])
def test_a_narrowing_step_follows_every_operator(dt, narrow):
  a, b, c = _tensor(dt), _tensor(dt), _tensor(dt)
  root = lower.apply('ADD', np.add, [lower.apply('MUL', np.multiply, [a, b]), c])
  prog, stream = _stream(root, dt)
  assert prog.cls == class_of(dt) and prog.out_dtype == _hip.sp_dtype(dt)
  assert stream == [('MUL', 0), narrow, ('ADD', 0), narrow]      # wrapped / rounded BEFORE the add, and after it


def test_casts_between_narrow_types_wrap_or_round():
  for src, dst, want in [(np.int8, np.uint8, ('TO_U8', 0)), (np.int8, np.uint16, ('TO_U8', 1)),
                         (np.int32, np.int16, ('TO_I32', 2)), (np.float32, np.float16, ('TO_F32', 1)),
                         (np.float64, np.uint32, ('TO_U8', 2)), (np.int16, np.float16, ('TO_F32', 1)),
                         (np.int8, np.bool_, ('TO_BOOL', 0)), (np.float16, np.bool_, ('TO_BOOL', 0)),
                         (np.uint8, np.int16, None), (np.int8, np.float16, None), (np.float16, np.float32, None),
                         (np.uint32, np.int64, None)]:
    root = lower.apply('ADD', np.add, [lower.cast(_tensor(src), dst), _tensor(dst)])
    _, stream = _stream(root, dst)
    first = stream[0] if stream[0][0].startswith('TO_') else None
    assert first == want, (src, dst, stream)


def test_programs_that_differ_in_the_selector_differ():
  a8, a16 = _tensor(np.int8), _tensor(np.int16)
  p8, _ = _stream(lower.apply('MUL', np.multiply, [a8, a8]), np.int8)
  p16, _ = _stream(lower.apply('MUL', np.multiply, [a16, a16]), np.int16)
  assert [p8.instr[i].op for i in range(2)] == [p16.instr[i].op for i in range(2)]
  assert p8.instr[1].c != p16.instr[1].c


def test_out_of_scope_kernels_refuse_the_new_types_by_name():
  for dt in NEW:
    with pytest.raises(TypeError, match='dtype %s is not supported by dot of the HIP tile backend .*astype' % dt):
      _hip.refuse_narrow(dt, 'dot')
  for dt in ALL[:6]:
    _hip.refuse_narrow(dt, 'dot')
