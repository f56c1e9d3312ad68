"""tests/extras_refusal_cases.py on the device: every row of the table through HipBackend.<op> and through the launcher
kernels.<op> on the same operands, which have to raise what the operation's check function raises -- the class and the
whole text -- before anything is launched or copied; then the valid call of every operation, for the shapes and dtypes
the table states.  Only refusals that come before the library is called go through here."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import kernels
from tests import extras_refusal_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _on_device(be, call):
  return [be.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a for a in call]


@pytest.mark.parametrize('op,defect', rc.CASES, ids=rc.CASE_IDS)
def test_the_backend_and_the_launcher_refuse_as_the_check_does(be, op, defect):
  call = defect.make(list(op.valid))
  want = rc.refusal(op.check, call)
  assert type(want) is defect.cls and defect.fragment in str(want), repr(want)
  call = _on_device(be, call)
  targets = [be.empty(shape, dtype) for shape, dtype in op.results] + [be.zeros((1,), np.int32)]
  before = be.launches
  got = rc.refusal(getattr(be, op.name), *call)
  assert type(got) is type(want) and str(got) == str(want), repr(got)
  if op.launch is not None:
    got = rc.refusal(op.launch, kernels, call, targets)
    assert type(got) is type(want) and str(got) == str(want), repr(got)
  assert be.launches == before


@pytest.mark.parametrize('op', rc.OPS, ids=lambda op: op.name)
def test_the_valid_call_runs(be, op):
  out = getattr(be, op.name)(*_on_device(be, op.valid))
  out = out if isinstance(out, tuple) else (out,)
  assert [(tuple(t.shape), be.dtype_of(t)) for t in out if t is not None] == op.results
  for t in out:
    if t is not None and be.dtype_of(t) == rc.F64:
      assert not np.any(np.isnan(t.numpy()))        # (the graph has +inf where there is no edge)
