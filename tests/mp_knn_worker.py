"""One rank of the two-rank NearestNeighbors test (launched by test_neighbors_example.py): 4 logical workers over 2
processes, so the row bands of X, the whole of Q and the bands' candidates all cross the ranks, and every rank must
come out with the same merged result."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import spartan_amd as sp  # noqa: E402
from oracle.np_backend import NumpyBackend  # noqa: E402
from spartan_amd.examples.sklearn.neighbors import NearestNeighbors  # noqa: E402
from tests import knn_cases as kc  # noqa: E402


def main():
  workers = int(sys.argv[1])
  use_hip = len(sys.argv) > 2 and sys.argv[2] == 'hip'
  world = sp.World.from_env(backend=os.environ.get('SPARTAN_TEST_BACKEND', 'socket'))
  assert world.size == 2
  if use_hip:
    world.staged = True
    sp.initialize('hip', num_workers=workers, world=world)
  else:
    sp.initialize(backend=NumpyBackend(), num_workers=workers, world=world)
  dtype = np.float32 if use_hip else np.float64
  nq, npts, d, k = 37, 1031, 33, 17
  before = dict(world.stats)
  q, x = kc.integer_case(nq, npts, d, dtype)
  want_d, want_i = kc.oracle(q, x, k)
  for hint in (None, (300, 17)):
    dist, ind = NearestNeighbors(k, 'auto').fit(sp.from_numpy(x, tile_hint=hint)).kneighbors(sp.from_numpy(q))
    np.testing.assert_array_equal(ind, want_i)
    assert dist.tobytes() == np.sqrt(want_d.astype(dtype)).tobytes()
  q, x = kc.real_case(nq, npts, d, dtype)
  dist, ind = NearestNeighbors(k, 'kd_tree').fit(x).kneighbors(q)
  kc.check_real(dist.astype(np.float64) ** 2, ind, q, x, k, d2_dtype=dtype, label='rank %d' % world.rank)
  assert world.stats['p2p_bytes'] > before['p2p_bytes'], 'nothing crossed the ranks?'
  world.barrier()
  print('RANK %d OK' % world.rank)
  sys.stdout.flush()


if __name__ == '__main__':
  main()
