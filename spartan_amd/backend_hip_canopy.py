"""The two tile bodies of canopy clustering as HipBackend has them (libspartan_hip_extras.so: sp_canopy, sp_pdf_label).
A mixin of its own beside backend_hip_extras.ExtrasTileBodies and its neighbours, whose public methods are fixed
tables; backend_hip.HipBackend inherits them all.  It uses the backend's memory methods (empty, contiguous, dtype_of,
to_numpy, _as_device), its `launches` counter and the stride helper of ExtrasTileBodies (_unit_rows) through `self`, and
keeps no state.

Each method reads top to bottom: check (tile_checks.check_canopy / check_pdf_label, which the launchers and the NumPy
bodies of examples/_canopy.py call too), allocate, normalise strides, launch.
"""
import numpy as np

from . import kernels, tile_checks
from .backend_hip_extras import _CopiesUncounted


class CanopyTileBodies(object):

  def canopy(self, x, t1, t2, chains=1, cap=None):
    """The reference's greedy canopy pass (canopy_clustering.py:33-65, without its `count > cf` filter) over the rows of
    a tile `x` [n, d], fp32 or fp64, as HOST arrays (centers [m, d] of x's dtype, counts [m] int64, rows [m] int64):
    all canopies of all chains, in chain order then creation order (sp_canopy: a chain's whole loop in one workgroup).
    The rows are cut into `chains` consecutive bands, band c = rows floor(c n / chains) .. floor((c + 1) n / chains) - 1,
    each with its own list of canopies.  Row after row: a canopy whose CREATING row is within t1 (squared distance,
    strict <) observes the row (count += 1, sum += row); a row within t2 of no creating row becomes a canopy.  centers
    are sum / count, rows the creating rows' indices in x.  The bytes of a band depend on its rows alone.
    The size of the result depends on the data, so the call reads the chains' canopy counts back: ONE wait for the
    device.  `cap`, the most canopies of a chain, defaults to min(the longest chain's rows, 1024); if a chain reports
    that it needs more, the call is repeated once with cap = the longest chain's rows, which always suffices.  x is not
    written; an operand whose elements do not lie next to each other is first copied, a row view of a wider array is
    taken as it is.  One launch (two with the retry).  Refusals: tile_checks.check_canopy's."""
    x = self._as_device(x)
    dt, n, d, t1, t2, chains, cap, _ = tile_checks.check_canopy(self.dtype_of(x), x.shape, t1, t2, chains, cap)
    with _CopiesUncounted(self):
      x = self._unit_rows(x)
    longest = max(-(-n // chains), 1)
    while True:
      slots = chains * cap
      centers, counts = self.empty((slots, d), dt), self.empty((slots,), np.int64)
      rows, num = self.empty((slots,), np.int64), self.empty((chains,), np.int64)
      self.launches += 1
      kernels.canopy(x, t1, t2, chains, cap, centers, counts, rows, num)
      num = np.asarray(self.to_numpy(num))              # (the one wait)
      if (num >= 0).all() or cap >= longest:
        break
      cap = longest
    assert (num >= 0).all(), num
    keep = np.concatenate([np.arange(c * cap, c * cap + m, dtype=np.int64) for c, m in enumerate(num)])
    centers, counts, rows = (np.asarray(self.to_numpy(t)) for t in (centers, counts, rows))
    return centers[keep], counts[keep], rows[keep]

  def pdf_label(self, x, centers):
    """The reference's _cluster_mapper (canopy_clustering.py:68-92) as a NEW device tensor [n] int32: per row of `x`
    [n, d] the lowest j at which 1 / (1 + |x_i - c_j|^2) is largest among `centers` [k, d], both fp32 or both fp64
    (sp_pdf_label); -1 with k = 0 and for a row whose every pdf is NaN.  Not an arg-min of the distance: 1 + d2 rounds,
    and of equal pdfs the lower index wins.  No operand is written; strided operands are first copied.  One launch
    (none for n = 0); never waits for the device.  Refusals: tile_checks.check_pdf_label's."""
    x, centers = self._as_device(x), self._as_device(centers)
    _, n, k, d = tile_checks.check_pdf_label([self.dtype_of(x), self.dtype_of(centers)], [x.shape, centers.shape])
    out = self.empty((n,), np.int32)
    if n:
      with _CopiesUncounted(self):
        x, centers = self._unit_rows(x), self._unit_rows(centers)
      self.launches += 1
      kernels.pdf_label(x, centers, out)
    return out
