"""The SGD matrix factorisation's tile body as HipBackend has it (libspartan_hip_extras.so: sp_sgd_mf).  A mixin of its
own beside backend_hip_extras.ExtrasTileBodies and backend_hip_svm.SvmTileBodies, whose public methods are fixed tables;
backend_hip.HipBackend inherits all three.  It uses the backend's memory methods (empty, dtype_of, _as_device) and its
`launches` counter through `self`, and keeps no state: the level schedule lives on the sparse tile (sparse.sgd_mf_plan).

The method reads top to bottom: check (tile_checks.check_sgd_mf, which the launcher and the NumPy body of
examples/_netflix.py call too), the tile's plan, launch.
"""
from . import kernels, tile_checks
from . import sparse as sparse_mod


class MfTileBodies(object):

  def sgd_mf(self, v, u, m, lr=None, want_error=False):
    """One pass of the reference's SGD (netflix_core.pyx, _sgd_inner) over the stored entries of the sparse tile `v`
    [rows, cols] in their stored order -- rows ascending, columns ascending inside a row -- updating `u` [rows, f] and
    `m` [cols, f], all fp32 or all fp64, IN PLACE: per entry (i, j, r)  d = r - dot(u_i, m_j),  u_i += (u_i d) lr,
    m_j += (m_j d) lr  with lr = float32(1e-5) unless given (sp_sgd_mf: level-scheduled, the bits of the sequential
    loop whatever the schedule).  Returns None, or with `want_error` a NEW tensor [nnz] of |d| per entry in the
    tile's entry order.  `u` and `m` are views with inner stride 1 (a row view of a wider array is taken as it is).
    The tile's level schedule is built on its first pass -- one copy of its structure to the host -- and kept on the
    tile.  The call counts as one launch (none for a tile without entries) and never waits for the device after the
    first pass.  Refusals: tile_checks.check_sgd_mf's; TypeError for a `v` that is not a sparse tile."""
    if not isinstance(v, sparse_mod.CsrTile):
      raise TypeError('sgd_mf: the ratings are a sparse tile, got %s' % type(v).__name__)
    u, m = self._as_device(u), self._as_device(m)
    dt, _, _, _, lr = tile_checks.check_sgd_mf([v.dtype, self.dtype_of(u), self.dtype_of(m)], v.shape, u.shape, m.shape, lr)
    for name, t in (('U', u), ('M', m)):
      if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError('sgd_mf: %s is updated in place and needs rows whose elements lie next to each other' % name)
    err = self.empty((v.nnz,), dt) if want_error else None
    if v.nnz:
      host, dev = sparse_mod.sgd_mf_plan(v)
      self.launches += 1
      kernels.sgd_mf(v.shape, v.data, dev, host, u, m, lr, abs_err=err)
    return err
