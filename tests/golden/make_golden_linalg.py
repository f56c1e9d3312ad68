"""Records tests/golden/cholesky_w4.npz: the reference's own blocked Cholesky (spartan/examples/cholesky.py) run at
4 workers on the N = 128 input of tests/linalg_cases.py, with the helpers of make_golden.py (the reference tree is
copied to a scratch directory, transliterated to Python 3 there and run in process; only the arrays are kept).

  python tests/golden/make_golden_linalg.py

One further Python-2 division is patched in the scratch copy: `tile_size = A.shape[0] / n` (cholesky.py:54)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import linalg_cases  # noqa: E402


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  mg.sub(os.path.join(mg.SCRATCH, 'spartan', 'examples', 'cholesky.py'),
         [('tile_size = A.shape[0] / n', 'tile_size = A.shape[0] // n')])
  mg.install_stubs()
  sp = mg.import_reference()
  from spartan.config import FLAGS
  from spartan.examples import cholesky
  a = np.array(linalg_cases.spd(128, np.float64))
  mg.start_cluster(sp, 4)
  FLAGS.num_workers = 4
  low = np.asarray(cholesky.cholesky(sp.from_numpy(a)).glom())
  np.savez_compressed(os.path.join(HERE, 'cholesky_w4.npz'), a=a, l=low)
  print('cholesky_w4.npz: L', low.dtype, low.shape, 'max |L - numpy| =', np.abs(low - np.linalg.cholesky(a)).max())


if __name__ == '__main__':
  main()
