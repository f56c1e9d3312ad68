"""Body of one rank of the two-rank logistic-gradient tests (launched by test_logreg.py on the oracle backend over
the socket transport, by test_logreg_gpu.py with the HIP backend on a shared GPU): the one-pass node with a link
(expr/rowdot.py) across ranks -- every rank's row tiles contribute a (d,) partial that joins the target like a
reduction's.  Prints 'RANK r OK n' on success."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import spartan_amd as sp  # noqa: E402
from oracle.np_backend import NumpyBackend  # noqa: E402
from spartan_amd.examples import logreg  # noqa: E402
from spartan_amd.expr.rowdot import LINK_EXP_RATIO, LINK_SIGMOID, RowDotColSumExpr  # noqa: E402


class _WithLinkKernel(NumpyBackend):
  """The oracle backend plus NumPy float32 statements of the two entry points of csrc/rowdot.hip (stand-ins: the
  rewrite never fires on a backend without them)."""

  def rowdot_colsum(self, x, w, y):
    return self.rowdot_link_colsum(x, w, y, 0)

  def rowdot_link_colsum(self, x, w, y, link):
    one = np.float32(1)
    t = x.astype(np.float32).dot(np.asarray(w, np.float32).reshape(-1, 1))
    if link == LINK_EXP_RATIO:
      e = np.exp(t)
      t = e / (e + one)
    elif link == LINK_SIGMOID:
      t = one / (one + np.exp(-t))
    return (x * (t if y is None else t - np.asarray(y).reshape(t.shape))).sum(0).astype(np.float32)


def main():
  workers = int(sys.argv[1])
  use_hip = len(sys.argv) > 2 and sys.argv[2] == 'hip'
  world = sp.World.from_env(backend=os.environ.get('SPARTAN_TEST_BACKEND', 'socket'))
  assert world.size == 2
  if use_hip:
    world.staged = True          # two ranks sharing GPU 0, HBM blobs staged through the host
    ctx = sp.initialize('hip', num_workers=workers, world=world)
  else:
    ctx = sp.initialize(backend=_WithLinkKernel(), num_workers=workers, world=world)
  rng = np.random.RandomState(11)
  xh, yh = (rng.rand(101, 32) - 0.5).astype(np.float32), rng.rand(101, 1).astype(np.float32)
  w = (rng.rand(32, 1) - 0.5).astype(np.float32)
  x64 = xh.astype(np.float64)
  e64 = np.exp(x64.dot(w.astype(np.float64)))
  want = (x64 * (e64 / (e64 + 1) - yh)).sum(0)             # what one process computes, in float64
  x, y = sp.Val(val=sp.from_numpy(xh).force()), sp.Val(val=sp.from_numpy(yh).force())
  ranks = sorted(set(ctx.rank_of(t.worker) for t in x.val.tiles.values()))
  assert ranks == [0, 1], ranks                            # row tiles on both ranks
  calls = []
  inner = ctx.backend.rowdot_link_colsum
  ctx.backend.rowdot_link_colsum = lambda *a: (calls.append(a[3]), inner(*a))[1]
  n = 0
  try:
    for build, link in ((lambda: logreg.gradient(x, y, w), LINK_EXP_RATIO),
                        (lambda: sp.sum(x * (1 / (1 + sp.exp(-sp.dot(x, w))) - y), axis=0), LINK_SIGMOID)):
      g = build().optimized()
      assert isinstance(g, RowDotColSumExpr) and g.link == link
      del calls[:]
      got = g.glom()
      mine = sum(1 for t in x.val.tiles.values() if ctx.rank_of(t.worker) == world.rank)
      assert calls == [link] * mine, (calls, mine)         # this rank's tiles, one call each
      np.testing.assert_allclose(got, want, rtol=2e-5)
      n += 1
  finally:
    del ctx.backend.rowdot_link_colsum
  # the driver across ranks: different np.random streams, the same start weights (rank 0 draws) and the same fit
  np.random.seed(100 + world.rank)
  w2 = logreg.fit(x, y, 2, alpha=1e-3)
  copies = world.all_gather_object(np.asarray(w2))
  np.testing.assert_array_equal(copies[0], copies[1])
  n += 1
  world.barrier()
  print('RANK %d OK %d' % (world.rank, n))
  sys.stdout.flush()


if __name__ == '__main__':
  main()
