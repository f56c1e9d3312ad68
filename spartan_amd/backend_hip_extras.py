"""The tile bodies outside the fused path as HipBackend has them (libspartan_hip_extras.so): the dense factorisations,
nearest neighbours, shortest paths, ALS, fuzzy k-means, LDA, naive Bayes, n-body, the affinity pair and the item
recommender's top-k.  One mixin, which backend_hip.HipBackend inherits; it uses the backend's memory methods (empty,
zeros, copy, contiguous, dtype_of, _as_device) and its `launches` counter and keeps no state of its own but syev_sweeps.

Every method reads top to bottom: check (tile_checks.check_<op>, which the launcher and the NumPy body under examples/
call too), allocate, normalise strides, launch.
"""
import numpy as np

from . import kernels, tile_checks


class _CopiesUncounted(object):
  """with _CopiesUncounted(backend): the copies that strided operands need inside the block belong to the call -- the
  call counts as the launches its method adds after the block, whatever its operands needed."""
  __slots__ = ('backend', 'before')

  def __init__(self, backend):
    self.backend, self.before = backend, backend.launches

  def __enter__(self):
    pass

  def __exit__(self, *exc):
    self.backend.launches = self.before


class ExtrasTileBodies(object):

  def _unit_rows(self, t):
    """A 2-D operand as a view with inner stride 1 and rows apart: the tensor itself where it is one (a row view of a
    wider array included), a contiguous copy otherwise."""
    rows_apart = t.shape[0] <= 1 or t.stride(0) >= t.shape[1]
    return t if (t.shape[1] <= 1 or t.stride(1) == 1) and rows_apart else self.contiguous(t)

  def _shared_rows(self, a, b):
    """Two 2-D operands of one shape as views with inner stride 1 and ONE row stride (the kernels that read a pair of
    lists take one for both): contiguous copies of both where theirs differ."""
    a, b = self._unit_rows(a), self._unit_rows(b)
    if a.shape[0] > 1 and a.stride(0) != b.stride(0):
      a, b = self.contiguous(a), self.contiguous(b)
    return a, b

  def potrf(self, t):
    """scipy.linalg.lapack.potrf(t, lower=1, clean=1)[0] as a NEW tensor: the Cholesky factor L of the symmetric
    positive definite fp32 / fp64 matrix `t` (its lower triangle is read), zero above the diagonal (sp_potrf;
    examples/cholesky.py:9-13).  numpy.linalg.LinAlgError, with LAPACK's words, if a leading minor is not positive
    definite -- learnt from one 4-byte copy to the host, the only point at which this call waits for the device."""
    t = self._as_device(t)
    _, n = tile_checks.check_potrf(self.dtype_of(t), t.shape)
    out = self.copy(t)           # (a strided view becomes contiguous here; the input is never written)
    if n == 0:
      return out
    info = self.empty((1,), np.int32)
    self.launches += 1
    kernels.potrf(out, info)
    order = int(info.numpy()[0])
    if order:
      raise np.linalg.LinAlgError('%d-th leading minor of the array is not positive definite' % order)
    return out

  def trsm_rlt(self, b, l):
    """x with x . l^T = b as a NEW tensor: `l` [n, n] lower triangular, `b` [m, n] (sp_trsm_rlt) -- scipy's
    dtrtrs(l, b.T, lower=1)[0].T (examples/cholesky.py:16-20), b . inv(l.T) without the inverse (ssvd/qr.py:40-43)."""
    b, l = self._as_device(b), self._as_device(l)
    tile_checks.check_trsm_rlt((self.dtype_of(b), self.dtype_of(l)), (b.shape, l.shape))
    out = self.copy(b)
    if out.numel():
      self.launches += 1
      kernels.trsm_rlt(out, self.contiguous(l))
    return out

  def syev(self, t):
    """(w, V) as NEW tensors: the eigenvalues of the symmetric fp32 / fp64 matrix `t` in ascending order and the
    eigenvectors as the columns of V, t . V = V . diag(w) (sp_syevj, two-sided Jacobi; LAPACK's syevd(t, lower=1): the
    lower triangle of `t` is read, `t` is not written).  numpy.linalg.LinAlgError if 64 sweeps do not converge (a NaN
    in `t`).  Waits for the device once per sweep (one word) and once for info; self.syev_sweeps holds the number of
    sweeps of the last call."""
    t = self._as_device(t)
    dt, n = tile_checks.check_syev(self.dtype_of(t), t.shape)
    w, v = self.empty((n,), dt), self.empty((n, n), dt)
    self.syev_sweeps = 0
    if n == 0:
      return w, v
    if n > 1 and t.stride(1) != 1:
      t = self.contiguous(t)
    info = self.empty((1,), np.int32)
    self.launches += 1
    self.syev_sweeps = kernels.syevj(t, w, v, info)
    if int(info.numpy()[0]):
      raise np.linalg.LinAlgError('Eigenvalues did not converge')
    return w, v

  def knn(self, queries, points, k, index_offset=0, splits=0):
    """(dist2, idx) as NEW tensors [nq, k]: for every row of `queries` [nq, d] the k rows of `points` [np, d] at the
    smallest squared Euclidean distance sum_j (q_j - x_j)^2 (computed in that form, in the operands' precision),
    ascending by (distance, index); idx (int64) = index_offset + row of `points`; +inf / -1 in the trailing slots when
    np < k (sp_knn: distance and selection in one pass, nothing of size nq x np is written).  Both operands fp32 or
    both fp64; 1 <= k <= 128.  splits: into how many ranges the points are cut (0: the library chooses); the result
    does not depend on it, bit for bit."""
    queries, points = self._as_device(queries), self._as_device(points)
    dt, nq, _, _, k, splits = tile_checks.check_knn((self.dtype_of(queries), self.dtype_of(points)),
                                                    (queries.shape, points.shape), k, splits)
    dist2, idx = self.empty((nq, k), dt), self.empty((nq, k), np.int64)
    if nq:
      self.launches += 1
      kernels.knn(self._unit_rows(queries), self._unit_rows(points), k, dist2, idx, index_offset, splits)
    return dist2, idx

  def knn_merge(self, cand_dist2, cand_idx, k):
    """(dist2, idx) as NEW tensors [nq, k]: per row the k smallest by (distance, index) of the m candidates
    (cand_dist2 fp32 / fp64, cand_idx int64, both [nq, m]); candidates with a negative index are padding, and so are
    the trailing slots of the result (+inf / -1) when fewer than k are left (sp_knn_merge)."""
    cand_dist2, cand_idx = self._as_device(cand_dist2), self._as_device(cand_idx)
    dt, nq, _, k = tile_checks.check_knn_merge((self.dtype_of(cand_dist2), self.dtype_of(cand_idx)),
                                               (cand_dist2.shape, cand_idx.shape), k)
    dist2, idx = self.empty((nq, k), dt), self.empty((nq, k), np.int64)
    if nq:
      cand_dist2, cand_idx = self._shared_rows(cand_dist2, cand_idx)
      self.launches += 1
      kernels.knn_merge(cand_dist2, cand_idx, k, dist2, idx)
    return dist2, idx

  def item_topk(self, targets, tnorm, sources, snorm, k, index_offset=0, splits=0):
    """(sim, idx) as NEW tensors [m, k]: for every column j of `targets` [users, m] the k columns i of `sources`
    [users, ns] of the largest cosine similarity nan_to_num(dot_u(t[u][j], s[u][i]) / (tnorm[j] * snorm[i])), ordered
    by (similarity descending, index ascending); idx (int64) = index_offset + column of `sources`; -inf / -1 in the
    trailing slots when ns < k (sp_item_topk: similarity and selection in one pass, nothing of size m x ns is written;
    include/spartan_hip_cf.h states the order of the arithmetic).  All four operands fp32 or all fp64; 1 <= k <= 128.
    A target is not excluded from its own list.  splits: into how many ranges the sources are cut (0: the library
    chooses); the result does not depend on it, nor on how the targets are banded, bit for bit.  Operands whose inner
    stride is not 1 are first copied contiguous; two column ranges of one table are taken as they are.  The library
    issues one kernel with one range and two with more (the second merges the ranges' candidates), and the call counts
    as that many launches -- none when m = 0.  Refusals: tile_checks.check_item_topk_operands'."""
    targets, tnorm, sources, snorm = (self._as_device(t) for t in (targets, tnorm, sources, snorm))
    dt, _, m, _, k, splits = tile_checks.check_item_topk_operands(
        [self.dtype_of(t) for t in (targets, tnorm, sources, snorm)], targets.shape, tnorm.shape, sources.shape,
        snorm.shape, k, splits)
    sim, idx = self.empty((m, k), dt), self.empty((m, k), np.int64)
    if m:
      with _CopiesUncounted(self):
        targets, sources = self._unit_rows(targets), self._unit_rows(sources)
        tnorm, snorm = self.contiguous(tnorm), self.contiguous(snorm)
      self.launches += kernels.item_topk(targets, tnorm, sources, snorm, k, sim, idx, index_offset, splits)
    return sim, idx

  def item_topk_merge(self, cand_sim, cand_idx, k):
    """(sim, idx) as NEW tensors [m, k]: per row the k best by (similarity descending, index ascending) of the
    candidates (cand_sim fp32 / fp64, cand_idx int64, both [m, cands]); candidates with a negative index are padding,
    and so are the trailing slots of the result (-inf / -1) when fewer than k are left (sp_item_topk_merge)."""
    cand_sim, cand_idx = self._as_device(cand_sim), self._as_device(cand_idx)
    dt, m, _, k = tile_checks.check_item_topk_merge((self.dtype_of(cand_sim), self.dtype_of(cand_idx)),
                                                    (cand_sim.shape, cand_idx.shape), k)
    sim, idx = self.empty((m, k), dt), self.empty((m, k), np.int64)
    if m:
      with _CopiesUncounted(self):
        cand_sim, cand_idx = self._shared_rows(cand_sim, cand_idx)
      self.launches += 1
      kernels.item_topk_merge(cand_sim, cand_idx, k, sim, idx)
    return sim, idx

  def apsp(self, t):
    """The matrix of shortest-path lengths as a NEW tensor: `t` [n, n], fp32 / fp64, holds the edge lengths of a
    directed graph (>= 0, +inf = no edge, the diagonal taken as 0; a symmetric `t` is an undirected graph); the result
    has +inf where there is no path and 0 on the diagonal (sp_apsp: blocked Floyd-Warshall in the (min, +) semiring;
    scipy.sparse.csgraph.shortest_path of the same weights, every path length the rounded sum of its edges).
    ValueError if an off-diagonal entry is negative or NaN -- learnt from one 4-byte copy to the host, the only point
    at which this call waits for the device."""
    t = self._as_device(t)
    _, n = tile_checks.check_apsp(self.dtype_of(t), t.shape)
    with _CopiesUncounted(self):
      out = self.copy(t)         # (a strided view becomes contiguous here; the input is never written)
    if n == 0:
      return out
    info = self.empty((1,), np.int32)
    self.launches += 1
    kernels.apsp(out, info)
    if int(info.numpy()[0]):
      raise ValueError('apsp: negative or NaN edge length')
    return out

  def graph_from_knn(self, dist, idx):
    """The dense undirected neighbour graph as a NEW tensor [n, n] of dist's dtype: +inf, 0 on the diagonal, and for
    every pair (i, idx[i][e]) of the lists dist (fp32 / fp64, >= 0) and idx (int64), both [n, k], the smallest weight
    stated for it in either direction, on both sides (sp_graph_from_knn); idx < 0 is padding.  What apsp takes."""
    dist, idx = self._as_device(dist), self._as_device(idx)
    dt, n, _ = tile_checks.check_graph_from_knn((self.dtype_of(dist), self.dtype_of(idx)), (dist.shape, idx.shape))
    w = self.empty((n, n), dt)
    if n:
      dist, idx = self._shared_rows(dist, idx)
      self.launches += 1
      kernels.graph_from_knn(dist, idx, w)
    return w

  def als_solve(self, ratings, factors, la, alpha, implicit=False, info=None):
    """One half-step of alternating least squares as a NEW tensor [m, f]: row i solves A_i x = b_i, built from row i of
    `ratings` [m, n] and `factors` [n, f] (sp_als_solve: accumulation, Cholesky and substitution fused, per row).
      explicit   A_i = sum_{r_ij != 0} y_j y_j^T + la |S_i| I,  b_i = sum r_ij y_j;  a row without ratings is exactly 0
      implicit   A_i = Y^T Y + sum_j alpha r_ij y_j y_j^T + la I,  b_i = sum_{r_ij > 0} (1 + alpha r_ij) y_j
    Both operands fp32 or both fp64; 1 <= f <= 64.  `info`: a device int32 tile of one element, zeroed by the caller and
    shared by as many calls as the caller likes; it receives 1 + the lowest failing row of the first call in which a
    system is not positive definite (that row of the result is NaN).  Without one the outcome is not reported.  The
    call counts as one launch when m > 0 and as none otherwise, and never waits for the device."""
    ratings, factors = self._as_device(ratings), self._as_device(factors)
    dt, m, _, f = tile_checks.check_als_solve((self.dtype_of(ratings), self.dtype_of(factors)),
                                              (ratings.shape, factors.shape))
    out = self.empty((m, f), dt)
    if m:
      if info is None:
        info = self.zeros((1,), np.int32)
      with _CopiesUncounted(self):
        ratings, factors = self._unit_rows(ratings), self._unit_rows(factors)
      self.launches += 1
      kernels.als_solve(ratings, factors, la, alpha, implicit, out, info)
    return out

  def fuzzy_step(self, points, centers, m, want_u=False, splits=0):
    """One iteration of the reference's fuzzy k-means on a row tile as NEW tensors (labels int64 [n], sums [k, d],
    wsum [k]), plus u [n, k] when `want_u` is set (sp_fuzzy_step: distances, memberships and the weighted sums fused;
    without `want_u` nothing of size n x k is allocated or written).  With dist_ij = |x_i - c_j| (1e-10 where it is 0)
    and p = dist ^ (1 / (m - 1)):  u_ij = p_ij / sum_j p_ij,  labels_i = the lowest j at the largest distance,
    w = u ^ m,  sums = w^T . points,  wsum_j = sum_i w_ij.  Both operands fp32 or both fp64; m finite and > 1; k >= 1.
    splits: into how many ranges the rows are cut (0: the library chooses); labels and u do not depend on it, bit for
    bit.  The call counts as one launch and never waits for the device."""
    points, centers = self._as_device(points), self._as_device(centers)
    dt, n, k, d, m, splits = tile_checks.check_fuzzy_step((self.dtype_of(points), self.dtype_of(centers)),
                                                          (points.shape, centers.shape), m, splits)
    labels, sums, wsum = self.empty((n,), np.int64), self.empty((k, d), dt), self.empty((k,), dt)
    u = self.empty((n, k), dt) if want_u else None
    with _CopiesUncounted(self):
      points, centers = self._unit_rows(points), self._unit_rows(centers)
    self.launches += 1
    kernels.fuzzy_step(points, centers, m, labels, sums, wsum, u=u, splits=splits)
    return (labels, sums, wsum, u) if want_u else (labels, sums, wsum)

  def lda_step(self, x, n, alpha, eta, iters, want_delta=True, want_doc_topics=True, splits=0):
    """The tile body of the reference's LDA (CVB0) on a tile of documents as NEW tensors (delta [k, V], doc_topics
    [D, k]; None in the place of one that is not wanted): `x` [V, D] terms x documents, `n` [k, V] the whole topic /
    term counts (sp_lda_step: the per-document loops fused, nothing of size V x D is allocated).  Per document gamma
    starts at 1 / k and is renewed `iters` times from q_tj = x_j p_tj / sum_t p_tj with p_tj = (n_tj + eta)
    (gamma_t + alpha) / (sum_j |n_tj| + eta V); doc_topics is the last gamma (a row of NaN for a document without a
    term), delta the sum over the documents of the last iteration's q.  Both operands fp32 or both fp64; 1 <= k <= 128,
    iters >= 1, alpha and eta finite and > 0.  splits: into how many ranges the documents are cut (0: the library
    chooses); doc_topics does not depend on it, bit for bit.  The call counts as one launch and never waits for the
    device."""
    x, n = self._as_device(x), self._as_device(n)
    dt, v, d, k, alpha, eta, iters, splits = tile_checks.check_lda_step(
        (self.dtype_of(x), self.dtype_of(n)), (x.shape, n.shape), alpha, eta, iters, splits)
    delta = self.empty((k, v), dt) if want_delta else None
    doc_topics = self.empty((d, k), dt) if want_doc_topics else None
    with _CopiesUncounted(self):
      x, n = self._unit_rows(x), self._unit_rows(n)
    self.launches += 1
    kernels.lda_step(x, n, alpha, eta, iters, delta=delta, doc_topics=doc_topics, splits=splits)
    return delta, doc_topics

  def nb_step(self, x, labels, label_size, splits=0):
    """The tile body of the reference's naive Bayes fit on a row tile as NEW tensors (S [label_size, d], df int64 [d],
    bad int64 [1]): `x` [m, d] documents x terms, `labels` int64 [m] or [m, 1] (sp_nb_step: normalisation and label
    sums fused, nothing of size m x d is allocated).  With r_i = sqrt(sum_j x_ij^2 / d):  S_lj = the sum over the rows
    with labels_i == l of x_ij / r_i, in row order;  df_j = the rows with x_ij > 0;  bad = 0, or 1 + the lowest row
    whose label is outside 0 .. label_size - 1 (it is left out of S and kept in df).  A row of zeros makes its label's
    row of S NaN.  `x` fp32 or fp64; 1 <= label_size <= 128.  splits: into how many ranges the rows are cut (0: the
    library chooses); df and bad do not depend on it.  The call counts as one launch when m > 0 and as none otherwise
    (the three results are then zeros), and never waits for the device."""
    x, labels = self._as_device(x), self._as_device(labels)
    dt = self.dtype_of(x)
    m, d, label_size = tile_checks.check_nb_operands(dt, x.shape, self.dtype_of(labels), labels.shape, label_size,
                                                     splits)
    if not m:
      return self.zeros((label_size, d), dt), self.zeros((d,), np.int64), self.zeros((1,), np.int64)
    s, df, bad = self.empty((label_size, d), dt), self.empty((d,), np.int64), self.empty((1,), np.int64)
    if labels.dim() == 2:
      labels = labels[:, 0]
    with _CopiesUncounted(self):
      if m > 1 and labels.stride(0) != 1:    # (a column of a wider array: the kernel reads the labels side by side)
        labels = self.contiguous(labels)
      x = self._unit_rows(x)
    self.launches += 1
    kernels.nb_step(x, labels, label_size, s, df, bad, splits=splits)
    return s, df, bad

  def nbody_accel(self, x, y, z, mass, r0, m, g=6.67384e-11, rmin=1.0, splits=0):
    """(ax, ay, az) as NEW tensors [m], the rows of one [3, m] array: the accelerations of bodies r0 .. r0 + m - 1 of
    `x`, `y`, `z`, `mass` [n] under the gravity of all n (sp_nbody_accel: every pair in registers, nothing of size
    n x n is allocated):  a_x[j] = sum over i != j of (g mass_i) / max(r_ij, rmin)^3 * (x_i - x_j), y and z alike.  All
    four fp32 or all fp64.  The bits of a[j] depend on body j, the n sources and (n, splits) alone, so a band of targets
    computed alone gives the bits the whole gives.  splits: into how many ranges the sources are cut (0: the library
    chooses from n).  A strided view is first made contiguous.  The library issues one kernel with one range and two
    with more (the second adds the ranges' partial sums), and the call counts as that many launches -- none when
    m = 0 -- and never waits for the device.  Refusals: tile_checks.check_nbody_operands'."""
    operands = [self._as_device(t) for t in (x, y, z, mass)]
    dt, _, r0, m, g, rmin, splits = tile_checks.check_nbody_operands(
        [self.dtype_of(t) for t in operands], [t.shape for t in operands], r0, m, g, rmin, splits)
    out = self.empty((3, m), dt)
    if m:
      with _CopiesUncounted(self):
        operands = [self.contiguous(t) for t in operands]
      self.launches += kernels.nbody_accel(*operands, r0, m, out[0], out[1], out[2], g, rmin, splits=splits)
    return out[0], out[1], out[2]

  def affinity_degree(self, x, y, metric='rbf', gamma=1.0):
    """The degrees D_i = sum_j a(x_i, y_j) of the rows of `x` [m, d] against ALL rows of `y` [n, d] as a NEW tensor [m]
    (sp_affinity_degree: the affinities stay in registers, nothing of size m x n is allocated).  metric: 'rbf'
    (a = exp(-gamma d2)), 'euclidean' (sqrt(d2)) or 'manhattan' (sum_f |x_f - y_f|), the distance in the difference
    form.  Both operands fp32 or both fp64.  The bits of D_i depend on row i of x and on y alone, so a band of rows
    computed alone gives the bits the whole gives.  The library issues one kernel, or two when n > 448 (the columns
    are then cut into ranges whose partial degrees a second kernel adds); the call counts as one launch when m > 0
    and as none otherwise, and never waits for the device.  Refusals: tile_checks.check_affinity_degree's."""
    x, y = self._as_device(x), self._as_device(y)
    dt, m, _, _, _, gamma = tile_checks.check_affinity_degree((self.dtype_of(x), self.dtype_of(y)), (x.shape, y.shape),
                                                              metric, gamma)
    deg = self.empty((m,), dt)
    if m:
      with _CopiesUncounted(self):
        x, y = self._unit_rows(x), self._unit_rows(y)
      self.launches += 1
      kernels.affinity_degree(x, y, metric, gamma, deg)
    return deg

  def affinity_matrix(self, x, r0, y, metric='rbf', gamma=1.0, scale=None):
    """The affinities of the rows of `x` [m, d] -- points r0 .. r0 + m - 1 of `y` [n, d] -- against all rows of `y` as a
    NEW tensor [m, n] (sp_affinity_matrix, one workgroup per 64 x 64 tile, written exactly once).  Without `scale` the
    plain a_ij; with `scale` [n] the normalised matrix of spectral clustering, a_ij * (scale[r0 + i] * scale[j]) with
    exactly 1 at j = r0 + i -- symmetric bit for bit when the bands are put together.  Metrics and dtypes as
    affinity_degree.  One kernel; the call counts as one launch when m > 0 and n > 0 and as none otherwise, and never
    waits for the device.  Refusals: tile_checks.check_affinity_matrix's (they come before the launch and before it is
    counted)."""
    x, y = self._as_device(x), self._as_device(y)
    given = (x, y) if scale is None else (x, y, self._as_device(scale))
    dt, m, n, _, _, gamma, r0 = tile_checks.check_affinity_matrix(
        [self.dtype_of(t) for t in given], [t.shape for t in given], r0, metric, gamma)
    out = self.empty((m, n), dt)
    with _CopiesUncounted(self):
      x, y = self._unit_rows(x), self._unit_rows(y)
      scale = None if scale is None else self.contiguous(given[2])
    self.launches += 1 if m and n else 0
    kernels.affinity_matrix(x, r0, y, metric, gamma, out, scale=scale)
    return out
