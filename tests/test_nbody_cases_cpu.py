"""tests/nbody_cases.py checked on the CPU: the oracle against a plain double loop, the NumPy restatement of the
kernel (examples/_nbody.accel_numpy) and the kernel's order rebuilt from pair_terms (nbody_cases.ordered_sum) against
the derived bound, the momentum the bound implies, that the bound is not vacuous, and the bindings of the library's
header.  Measured shares of the bounds are printed before each assertion (pytest -s)."""
import os
import re

import numpy as np
import pytest

from spartan_amd import _hip, tile_checks
from spartan_amd.examples import _nbody
from tests import nbody_cases as nc

DTYPES = (np.float32, np.float64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_oracle_agrees_with_a_plain_double_loop():
  x, y, z, mass = nc.unit_case(5, np.float64)
  a, s = nc.oracle(x, y, z, mass, nc.UNIT_G, nc.UNIT_RMIN)
  for j in range(5):
    want, total = [nc.LD(0)] * 3, [nc.LD(0)] * 3
    for i in range(5):
      if i == j:
        continue
      d = [nc.LD(v[i]) - nc.LD(v[j]) for v in (x, y, z)]
      r = max(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), nc.LD(np.float64(nc.UNIT_RMIN)))
      for k in range(3):
        t = nc.LD(nc.UNIT_G) * nc.LD(mass[i]) * d[k] / (r * r * r)
        want[k], total[k] = want[k] + t, total[k] + abs(t)
    for k in range(3):
      assert abs(a[k, j] - want[k]) <= 8 * np.finfo(nc.LD).eps * total[k]
      assert abs(s[k, j] - total[k]) <= 8 * np.finfo(nc.LD).eps * total[k]


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('n,kind', ((2, 'random'), (5, 'random'), (65, 'random'), (130, 'placed'), (257, 'random')))
def test_the_restatement_and_the_rebuilt_order_meet_the_bound(n, kind, dtype):
  x, y, z, mass = nc.unit_case(n, dtype, kind=kind)
  want = nc.oracle(x, y, z, mass, nc.UNIT_G, nc.UNIT_RMIN)
  got = _nbody.accel_numpy(x, y, z, mass, 0, n, nc.UNIT_G, nc.UNIT_RMIN)
  nc.check_accel(got, x, y, z, mass, nc.UNIT_G, nc.UNIT_RMIN, 'accel_numpy n=%d %s' % (n, np.dtype(dtype).name), want=want)
  for splits in (0, 1, 3):
    got = nc.ordered_accel(x, y, z, mass, nc.UNIT_G, nc.UNIT_RMIN, splits)
    nc.check_accel(got, x, y, z, mass, nc.UNIT_G, nc.UNIT_RMIN,
                   'ordered_sum n=%d splits=%d %s' % (n, splits, np.dtype(dtype).name), want=want)
  # a band alone: the bits of the whole
  lo, m = (n // 3, min(9, n - n // 3))
  band = _nbody.accel_numpy(x, y, z, mass, lo, m, nc.UNIT_G, nc.UNIT_RMIN)
  whole = _nbody.accel_numpy(x, y, z, mass, 0, n, nc.UNIT_G, nc.UNIT_RMIN)
  for b, w in zip(band, whole):
    assert b.tobytes() == w[lo:lo + m].tobytes()


def test_the_placed_pairs_are_what_they_say():
  for dtype in DTYPES:
    n = 130
    x, y, z, mass = nc.unit_case(n, dtype, kind='placed')
    (a, b), (c, d) = nc.placed_pairs(n)
    tx, ty, tz = _nbody.pair_terms(x, y, z, mass, a, nc.UNIT_G, nc.UNIT_RMIN)
    dt = np.dtype(dtype)
    rmin = dt.type(nc.UNIT_RMIN)
    w = (dt.type(nc.UNIT_G) * mass[b]) / ((rmin * rmin) * rmin)           # the pair at rmin / 2 uses rmin
    assert tx[b] == w * (x[b] - x[a]) and ty[b] == 0 and tz[b] == 0
    for t in _nbody.pair_terms(x, y, z, mass, c, nc.UNIT_G, nc.UNIT_RMIN):
      assert t[d] == 0 and not np.signbit(t[d])                           # the coincident pair adds exactly +0


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_momentum_is_within_the_bound_it_implies(dtype):
  """sum_j m_j a_j = 0 exactly (t_ij m_j = -t_ji m_i), so |sum_j m_j a_j| <= sum_j m_j gamma S_j plus the roundings of
  this very sum, formed in longdouble here."""
  n = 130
  x, y, z, mass = nc.unit_case(n, dtype)
  a, s = nc.oracle(x, y, z, mass, nc.UNIT_G, nc.UNIT_RMIN)
  got = _nbody.accel_numpy(x, y, z, mass, 0, n, nc.UNIT_G, nc.UNIT_RMIN)
  u = nc.unit_roundoff(dtype)
  for k in range(3):
    p = (np.asarray(mass, nc.LD) * np.asarray(got[k], nc.LD)).sum()
    # (the oracle's own g m_i m_j products differ from the kernel's T(g) m_i by the rounding of that product: u per term)
    bound = (np.asarray(mass, nc.LD) * (nc.gamma(n, dtype) + u) * s[k]).sum()
    print('momentum %s component %d: %.3g of its bound' % (np.dtype(dtype).name, k, abs(p) / bound))
    assert abs(p) <= bound


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_bound_is_not_vacuous(dtype):
  n = 65
  x, y, z, mass = nc.unit_case(n, dtype)
  a, s = nc.oracle(x, y, z, mass, nc.UNIT_G, nc.UNIT_RMIN)
  for j in (0, 33, 64):
    terms = [np.array(t) for t in _nbody.pair_terms(x, y, z, mass, j, nc.UNIT_G, nc.UNIT_RMIN)]
    i = (j + 7) % n
    for k in range(3):
      terms[k][i] = 0                                                     # one term dropped
      got = nc.ordered_sum(terms[k], n)
      assert abs(nc.LD(got) - a[k, j]) > nc.gamma(n, dtype) * s[k, j]


def test_ranges_are_chosen_from_n_alone():
  assert nc.ranges_of(1000, 0) * -(-1000 // 64) >= 256                    # n = 1000: a workgroup per CU at the least
  assert nc.ranges_of(65536, 0) == 1 and nc.ranges_of(10 ** 6, 0) == 1
  assert [nc.ranges_of(n, 0) for n in (1, 64, 65, 130, 600, 8192)] == [1, 1, 2, 3, 10, 8]
  assert [nc.ranges_of(600, s) for s in (1, 2, 3, 64)] == [1, 2, 3, 10]


def test_the_header_declares_what_is_bound():
  text = open(os.path.join(ROOT, 'include', 'spartan_hip_nbody.h')).read()
  names = sorted(set(re.findall(r'\b(sp_nbody\w+)\s*\(', text)))
  assert names == sorted(_hip.EXPORTS_NBODY) == ['sp_nbody_accel', 'sp_nbody_accel_workspace_bytes']
  for name, value in (('SP_NBODY_BLOCK', nc.BLOCK), ('SP_NBODY_WAVES', nc.CLASSES), ('SP_NBODY_WORKGROUPS', nc.WORKGROUPS)):
    assert re.search(r'#define %s %d\b' % (name, value), text)


def test_operand_refusals():
  f32, f64 = np.dtype(np.float32), np.dtype(np.float64)
  ok = ([f64] * 4, [(9,)] * 4, 0, 9, 1.0, 1.0)
  assert tile_checks.check_nbody_operands(*ok)[:4] == (f64, 9, 0, 9)
  for bad in (np.int32, np.float16, np.complex128, object):
    with pytest.raises(TypeError, match='astype first'):
      tile_checks.check_nbody_operands([f64, f64, np.dtype(bad), f64], [(9,)] * 4, 0, 9, 1.0, 1.0)
  with pytest.raises(TypeError, match='two dtypes.*astype first'):
    tile_checks.check_nbody_operands([f64, f64, f32, f64], [(9,)] * 4, 0, 9, 1.0, 1.0)
  for shapes in ([(9,), (9,), (8,), (9,)], [(9, 1)] * 4, [(3, 3)] * 4):
    with pytest.raises(ValueError, match='1-D and of equal length'):
      tile_checks.check_nbody_operands([f64] * 4, shapes, 0, 1, 1.0, 1.0)
  for r0, m in ((-1, 2), (0, 10), (9, 1), (3, -1)):
    with pytest.raises(ValueError, match='not among'):
      tile_checks.check_nbody_operands([f64] * 4, [(9,)] * 4, r0, m, 1.0, 1.0)
  with pytest.raises(ValueError, match='splits'):
    tile_checks.check_nbody_operands([f64] * 4, [(9,)] * 4, 0, 9, 1.0, 1.0, splits=-1)
  for g in (float('nan'), float('inf'), -float('inf')):
    with pytest.raises(ValueError, match='g = '):
      tile_checks.check_nbody_operands([f64] * 4, [(9,)] * 4, 0, 9, g, 1.0)
  with pytest.raises(ValueError, match='g = '):
    tile_checks.check_nbody_operands([f32] * 4, [(9,)] * 4, 0, 9, 1e300, 1.0)         # not finite in float32
  for rmin in (0.0, -1.0, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='rmin'):
      tile_checks.check_nbody_operands([f64] * 4, [(9,)] * 4, 0, 9, 1.0, rmin)
  with pytest.raises(ValueError, match='rmin'):
    tile_checks.check_nbody_operands([f32] * 4, [(9,)] * 4, 0, 9, 1.0, 1e-60)         # 0 in float32
