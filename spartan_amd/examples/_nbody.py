"""The tile body of the n-body driver: backend.nbody_accel where the backend has it (HipBackend: sp_nbody_accel), NumPy
on host arrays otherwise -- the same arithmetic per pair, operation for operation in the arrays' dtype
(include/spartan_hip_nbody.h), which keeps the driver runnable on a backend of plain NumPy tiles.  Both paths refuse
through one function, tile_checks.check_nbody_operands (the launcher and HipBackend.nbody_accel call it too)."""
import numpy as np

from .. import context, tile_checks
from ..array import distarray

check_operands = tile_checks.check_nbody_operands
G = 6.67384e-11       # m^3 / (kg s^2): the reference's constant


def pair_terms(x, y, z, mass, j, g, rmin):
  """(tx, ty, tz), each [n] in the arrays' dtype T: what every source i adds to target j, as the kernel forms it --
  dx = x_i - x_j, q = (dx dx + dy dy) + dz dz, r = sqrt(q) clamped from below at T(rmin) (a NaN stays),
  w = (T(g) mass_i) / ((r r) r), the term w dx -- and +0 for i == j."""
  dt = x.dtype
  with np.errstate(all='ignore'):
    dx, dy, dz = x - x[j], y - y[j], z - z[j]
    q = (dx * dx + dy * dy) + dz * dz
    r = np.sqrt(q)
    r = np.where(r < dt.type(rmin), dt.type(rmin), r)
    w = (dt.type(g) * mass) / ((r * r) * r)
    terms = [w * dx, w * dy, w * dz]
  for t in terms:
    t[j] = 0
    assert t.dtype == dt
  return tuple(terms)


def accel_numpy(x, y, z, mass, r0, m, g, rmin):
  """(ax, ay, az), each [m]: the sums over all sources of pair_terms for the targets r0 .. r0 + m - 1, formed as
  [sources, targets] arrays in blocks of at most 256 targets.  The sum over the sources is NumPy's (pairwise over a
  column), in another order than the kernel's; like the kernel's it does not depend on the band the target is in."""
  dt = x.dtype
  out = [np.zeros((m,), dt) for _ in range(3)]
  with np.errstate(all='ignore'):
    gm = dt.type(g) * mass
    for lo in range(r0, r0 + m, 256):
      hi = min(lo + 256, r0 + m)
      dx, dy, dz = (v[:, None] - v[None, lo:hi] for v in (x, y, z))
      q = (dx * dx + dy * dy) + dz * dz
      r = np.sqrt(q)
      r = np.where(r < dt.type(rmin), dt.type(rmin), r)
      w = gm[:, None] / ((r * r) * r)
      own = np.arange(lo, hi)
      for o, d in zip(out, (dx, dy, dz)):
        t = w * d
        t[own, own - lo] = 0
        # (a column at a time, so that a target's sum is the same whatever block it is in)
        o[lo - r0:hi - r0] = [np.ascontiguousarray(t[:, c]).sum() for c in range(hi - lo)]
  assert all(o.dtype == dt for o in out)
  return tuple(out)


def nbody_accel(x, y, z, mass, r0, m, g=G, rmin=1.0, splits=0):
  """(ax, ay, az) as new tiles [m]: the accelerations of bodies r0 .. r0 + m - 1 of `x`, `y`, `z`, `mass` [n], all
  float32 or all float64.  TypeError ("astype first") for other or mixed dtypes, ValueError for shapes that do not
  fit, targets that are not among the bodies, a g that is not finite or an rmin that is not finite and > 0."""
  operands = (x, y, z, mass)
  if any(isinstance(t, distarray.Absent) for t in operands):
    dt, _, _, m, _, _, _ = check_operands([t.dtype for t in operands], [t.shape for t in operands], r0, m, g, rmin, splits)
    return tuple(distarray.Absent((m,), dt) for _ in range(3))
  be = context.get().backend
  fn = getattr(be, 'nbody_accel', None)
  if fn is not None:
    return fn(x, y, z, mass, r0, m, g=g, rmin=rmin, splits=splits)
  host = [np.asarray(be.to_numpy(t)) for t in operands]
  _, _, r0, m, g, rmin, _ = check_operands([t.dtype for t in host], [t.shape for t in host], r0, m, g, rmin, splits)
  return accel_numpy(*host, r0, m, g, rmin)
