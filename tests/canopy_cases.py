"""The inputs of the canopy clustering tests and of tests/golden/make_golden_canopy.py, and the recorded reference.

golden_input(s): setting s of SETTINGS = (d, spread, t1, t2) is 160 rows around 6 blobs,
    rng = RandomState(7); blobs = rng.rand(6, d); x = blobs[rng.randint(0, 6, 160)] + spread * rng.randn(160, d)
in float64, clustered at WORKERS = 4 row bands of 40 with cf = CF.  tests/golden/canopy_w4.npz holds, per setting s:
    band_s_b  (b = 0 .. 3)     the reference's own _canopy_mapper on band b: the means of its canopies with count > cf
    centers_s                  the reference's find_centers on the bands in ascending order
    labels_s                   the reference's _cluster_mapper on the whole input with those centres
    whole_run_s, run_labels_s  1 and the labels of the reference's canopy_cluster itself if it evaluated, else 0 and
                               an empty array; run_order_s is then the order in which it took the bands
The recording script asserts that every distance the loops meet is at least 1e-6 (relative) away from t1 and t2 and that
the two largest pdfs of every row differ by at least 1e-9: neither the order of a sum nor a last-bit difference can
change a decision, so float64 results are compared byte for byte."""
import os

import numpy as np

SETTINGS = ((3, 0.12, 0.1, 0.1), (3, 0.12, 0.3, 0.1), (3, 0.12, 0.05, 0.2), (19, 0.05, 0.3, 0.1))
ROWS, BLOBS, WORKERS, CF = 160, 6, 4, 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'canopy_w4.npz')


def golden_input(s):
  """(x [160, d] float64, t1, t2) of setting s."""
  d, spread, t1, t2 = SETTINGS[s]
  rng = np.random.RandomState(7)
  blobs = rng.rand(BLOBS, d)
  x = blobs[rng.randint(0, BLOBS, ROWS)] + spread * rng.randn(ROWS, d)
  return np.ascontiguousarray(x), t1, t2


def bands(n=ROWS, workers=WORKERS):
  """The row bands (lo, hi) of divup(n, workers) rows."""
  step = -(-n // workers)
  return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def chain_rows(n, chains):
  """The rows (lo, hi) of every chain: sp_canopy's cut."""
  return [(c * n // chains, (c + 1) * n // chains) for c in range(chains)]


_golden = None


def golden():
  global _golden
  if _golden is None:
    with np.load(GOLDEN) as z:
      _golden = {k: z[k] for k in z.files}
  return _golden


def same(a, b):
  """Equal shape, dtype and bytes."""
  a, b = np.asarray(a), np.asarray(b)
  return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
