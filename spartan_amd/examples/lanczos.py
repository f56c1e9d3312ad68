"""Lanczos iteration for the leading eigenpairs (interface and order of operations of the reference's
spartan/examples/lanczos.py: `solve(A, AT, desired_rank, is_symmetric)` -> (d, s)).

As in the reference only the matrix-vector product is distributed: `expr.dot(A, v)` (or `dot(AT, dot(A, v))` when the
matrix is not symmetric), one fused multiply-reduce launch per row tile of the matrix, glommed to the host.  Everything
else is float64 NumPy on the driver whatever the matrix's dtype -- the start vector ones / sqrt(n), two steps more than
asked for, full reorthogonalisation against every earlier vector (a projection that is exactly 0 is skipped),
numpy.linalg.eig of the tridiagonal matrix, the Ritz pairs sorted by descending absolute value, s = V . v.  The vector
is handed to the product in the matrix's dtype.

Deviation from the reference: a beta of exactly 0 (breakdown: the Krylov space is exhausted) raises
numpy.linalg.LinAlgError; the reference divides by it silently and returns NaN."""
import numpy as np

from .. import expr


def ritz_pairs(product, n, rank):
  """(theta [rank], Y [n, rank]) after rank + 2 Lanczos steps with `product`, a function from a float64 vector [n] to
  the float64 vector matrix . v: the host part of `solve`, whatever computes the product."""
  steps = int(rank) + 2
  q, q_before = np.ones(n) / np.sqrt(n), np.zeros(n)
  diag, off = np.zeros(steps), np.zeros(steps + 1)          # off[i] couples steps i - 1 and i; off[0] = 0
  basis = np.zeros((n, steps))

  for i in range(steps):
    w = product(q)
    diag[i] = np.dot(w, q)
    w = w - diag[i] * q - off[i] * q_before
    for t in range(i):                                      # against every earlier vector; an exact 0 is skipped
      overlap = np.dot(w, basis[:, t])
      if overlap != 0.0:
        w -= overlap * basis[:, t]
    off[i + 1] = np.linalg.norm(w, 2)
    basis[:, i] = q
    if i + 1 < steps:                                       # (after the last step nothing divides by it)
      if off[i + 1] == 0.0:
        raise np.linalg.LinAlgError('lanczos.solve: breakdown at step %d of %d (beta = 0): the Krylov space of the '
                                    'start vector is exhausted' % (i + 1, steps))
      q_before, q = q, w / off[i + 1]

  small = np.diag(diag) + np.diag(off[1:steps], 1) + np.diag(off[1:steps], -1)
  theta, vectors = np.linalg.eig(small)
  order = np.argsort(np.abs(theta))[::-1][:steps - 2]       # descending absolute value, the two extra ones dropped
  return theta[order], np.dot(basis, vectors[:, order])


def solve(A, AT, desired_rank, is_symmetric=False):
  """(d [desired_rank], s [n, desired_rank]): the Ritz values of largest absolute value, descending, of A (or of
  AT . A when `is_symmetric` is false) after desired_rank + 2 Lanczos steps, and their Ritz vectors."""
  n = int(A.shape[1])
  dtype = np.dtype(A.dtype)

  def product(v):
    column = expr.from_numpy(v.reshape(n, 1).astype(dtype))
    w = expr.dot(A, column) if is_symmetric else expr.dot(AT, expr.dot(A, column))
    return np.asarray(w.optimized().glom()).reshape(n).astype(np.float64)

  return ritz_pairs(product, n, desired_rank)
