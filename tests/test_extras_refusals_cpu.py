"""tests/extras_refusal_cases.py on the CPU: every row of the table through the operation's check function
(spartan_amd/tile_checks.py) and through its NumPy body under examples/, which has to raise the same class with the
identical text; the valid call passes the check with the sizes the table states and runs through the NumPy body."""
import inspect

import numpy as np
import pytest

from tests import extras_refusal_cases as rc


@pytest.fixture(scope='module')
def numpy_backend():
  import spartan_amd as sp
  from oracle.np_backend import NumpyBackend
  sp.initialize(backend=NumpyBackend(), num_workers=1)
  yield
  sp.shutdown()


@pytest.mark.parametrize('op,defect', rc.CASES, ids=rc.CASE_IDS)
def test_the_check_and_the_numpy_body_refuse_alike(numpy_backend, op, defect):
  call = defect.make(list(op.valid))
  refused = rc.refusal(op.check, call)
  assert type(refused) is defect.cls and defect.fragment in str(refused), repr(refused)
  body = rc.body_of(op)
  taken = len(inspect.signature(body).parameters)
  if defect.arg < taken:                 # (a body without ranges has no `splits`)
    by_body = rc.refusal(body, *call[:taken])
    assert type(by_body) is defect.cls and str(by_body) == str(refused), repr(by_body)


@pytest.mark.parametrize('op', rc.OPS, ids=lambda op: op.name)
def test_the_valid_call_passes(numpy_backend, op):
  assert op.check(list(op.valid)) == op.sizes
  body = rc.body_of(op)
  out = body(*op.valid[:len(inspect.signature(body).parameters)])
  out = out if isinstance(out, tuple) else (out,)
  assert [(np.shape(t), np.asarray(t).dtype) for t in out if t is not None] == op.results


def test_every_operation_is_in_the_table():
  from spartan_amd import backend_hip_extras
  methods = [n for n, f in vars(backend_hip_extras.ExtrasTileBodies).items() if inspect.isfunction(f) and n[0] != '_']
  assert sorted(methods) == sorted(op.name for op in rc.OPS)
