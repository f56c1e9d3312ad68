"""The swaption pricer's tile body as HipBackend has it (libspartan_hip_extras.so: sp_lmm_swaption).  A mixin of its own
beside backend_hip_extras.ExtrasTileBodies, whose public methods are a fixed table; backend_hip.HipBackend inherits
both.  It uses the backend's memory methods (empty, contiguous, dtype_of, _as_device), its `launches` counter and the
stride helper of ExtrasTileBodies (_unit_rows) through `self`, and keeps no state.

The method reads top to bottom: check (tile_checks.check_lmm_swaption, which the launcher and the NumPy body of
examples/_swaption.py call too), allocate, normalise strides, launch.
"""
from . import kernels, tile_checks
from .backend_hip_extras import _CopiesUncounted


class LmmTileBodies(object):

  def lmm_swaption(self, eps, maturities, lamb, delta=0.5, f0=0.06, theta=0.06):
    """The discounted payoffs of one European payer swaption under the LIBOR market model (swaption.py:47-97) as a NEW
    tensor [n]: `eps` [S, n] fp32 or fp64 holds the draws of n antithetic pairs of paths for S time steps; every pair
    walks K = `maturities` forward rates from `f0` through the S steps of length `delta` with volatility `lamb`, once
    with its draws and once with their negatives, prices the swap with strike `theta` over the maturities S .. K - 1
    and discounts it; the output is the mean of the two (sp_lmm_swaption: all steps in one kernel, the rates on chip,
    every draw read once per sign).  The bits of a pair depend on its column and the scalars alone: a band of columns
    computed alone gives the bits of the whole.  `eps` is not written.  A column view of a wider array is taken as it
    is; anything else that is not unit-stride along the rows is first copied.  The call counts as one launch -- none
    for n = 0 -- and never waits for the device.  Refusals: tile_checks.check_lmm_swaption's."""
    eps = self._as_device(eps)
    dt, n, _, k, lamb, delta, f0, theta = tile_checks.check_lmm_swaption(self.dtype_of(eps), eps.shape, maturities, lamb,
                                                                         delta, f0, theta)
    out = self.empty((n,), dt)
    if n:
      with _CopiesUncounted(self):
        eps = self._unit_rows(eps)
      self.launches += 1
      kernels.lmm_swaption(eps, k, lamb, delta, f0, theta, out)
    return out
