"""The linear SVM's tile body as HipBackend has it (libspartan_hip_extras.so: sp_svm_dca).  A mixin of its own beside
backend_hip_extras.ExtrasTileBodies, whose public methods are a fixed table; backend_hip.HipBackend inherits both.  It
uses the backend's memory methods (empty, contiguous, dtype_of, _as_device), its `launches` counter and the stride
helper of ExtrasTileBodies (_unit_rows) through `self`, and keeps no state.

The method reads top to bottom: check (tile_checks.check_svm_dca, which the launcher and the NumPy body of
examples/_svm.py call too), allocate, normalise strides, launch.
"""
from . import kernels, tile_checks
from .backend_hip_extras import _CopiesUncounted


class SvmTileBodies(object):

  def svm_dca(self, x, y, alpha, w0, scaled_lambda, chains=1, want_w=False):
    """One pass of the reference's dual coordinate ascent (disdca_svm.py:5-25) over the rows of a tile as a NEW tensor
    alpha [m, 1], or (alpha, w [chains, d]) when `want_w` is set: `x` [m, d], `y` and `alpha` [m] or [m, 1], `w0` [d] or
    [d, 1], all fp32 or all fp64 (sp_svm_dca: the whole loop over the rows in one kernel, w on chip).  The rows are cut
    into `chains` consecutive bands, band c = rows floor(c m / chains) .. floor((c + 1) m / chains) - 1; every band
    starts from w = w0 and, row after row,  g = (y_i - x_i . w) / (s x_i . x_i),  dl = y_i clamp(y_i (g + a_i), 0, 1)
    - a_i,  w += (x_i s) dl,  a_i += dl  with s = scaled_lambda.  w row c is what band c ends with (w0 for a band
    without rows).  The bits of a band depend on its rows, w0 and d alone: `chains` calls on the bands give the bits of
    one call.  No operand is written.  Operands whose elements do not lie next to each other are first copied; a row
    view of a wider array is taken as it is.  The call counts as one launch -- none when there is nothing to write (m = 0
    without `want_w`) -- and never waits for the device.  Refusals: tile_checks.check_svm_dca's."""
    x, y, alpha, w0 = (self._as_device(t) for t in (x, y, alpha, w0))
    dt, m, d, scaled_lambda, chains = tile_checks.check_svm_dca(
        [self.dtype_of(t) for t in (x, y, alpha, w0)], [t.shape for t in (x, y, alpha, w0)], scaled_lambda, chains)
    out = self.empty((m, 1), dt)
    w = self.empty((chains, d), dt) if want_w else None
    if m or want_w:
      with _CopiesUncounted(self):
        x = self._unit_rows(x)
        y, alpha, w0 = (t if t.numel() <= 1 or t.stride(0) == 1 else self.contiguous(t) for t in (y, alpha, w0))
      self.launches += 1
      kernels.svm_dca(x, y, alpha, w0, scaled_lambda, chains, out, w_out=w)
    return (out, w) if want_w else out
