"""The NumPy tile bodies of the spectral-clustering driver (examples/_spectral.py: degree_numpy, matrix_numpy) against
the longdouble oracle and the derived bound of tests/spectral_cases.py, and against the reference's own mapper outputs
(tests/golden/spectral_w4.npz).

The bodies use the kernel's recipe in the tile's dtype, so what holds for them at these shapes is what the GPU tests ask
of the kernels (tests/test_spectral_gpu.py, the same shapes).  A share of the bound above one half HERE would mean the
derivation is wrong, and is asserted for D and L at every shape and for A everywhere but 'euclidean' and 'manhattan' at
d = 2 and 3 (there a_ij carries three to five roundings, the bound counts exactly those, and single pairs come close
to it: up to 0.86 at d = 2) -- in float32
'rbf' with NumPy's own float32 exp, which is up to 2.8 u off by itself, replaced by one that is rounded once.  The full
bound is asserted for everything as computed.

Against the golden, in float64 (the golden's points are float64): |ours - golden| <= bound x |oracle| for A, D and L, the
bound of the issue (the reference's own outputs carry roundings of their own, which this does not allow for: at this
input ours and the reference's A and D have the same bits and L differs by 0.04 of the bound at most)."""
import os

import numpy as np
import pytest

from spartan_amd.examples import _spectral
from tests import spectral_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = (np.float32, np.float64)


def _bodies(y, r0, m, metric, gamma=1.0):
  """(D of the band, D of all points, A, L) from the NumPy bodies, as the driver chains them."""
  x = y[r0:r0 + m]
  deg_all = _spectral.degree_numpy(y, y, metric, gamma)
  deg = _spectral.degree_numpy(x, y, metric, gamma)
  a = _spectral.matrix_numpy(x, r0, y, metric, gamma)
  lap = _spectral.matrix_numpy(x, r0, y, metric, gamma, scale=sc.scale_of(deg_all))
  return deg, deg_all, a, lap


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('metric', sc.METRICS)
@pytest.mark.parametrize('shape', sc.SHAPES, ids=lambda s: '%dx%dx%d+%d' % s)
def test_the_numpy_bodies_use_under_half_of_the_bound(shape, metric, dtype):
  m, n, d, r0 = shape
  y = sc.case(n, d, np.dtype(dtype))
  want = sc.oracle_of_case(n, d, np.dtype(dtype), metric)
  deg, deg_all, a, lap = _bodies(y, r0, m, metric)
  assert deg.tobytes() == deg_all[r0:r0 + m].tobytes()          # a band's degrees are the whole's
  shares = sc.check(y, r0, m, metric, want, deg=deg, a=a, lap=lap,
                    label='numpy %s %s %s' % (shape, metric, np.dtype(dtype).name))
  if metric == 'rbf' and np.dtype(dtype) == np.float32:
    # NumPy's vectorised float32 exp alone is up to 2.8 u off (measured on these arguments against longdouble), 0.7 of
    # the 4 u the bound grants EXP.  What the half-of-the-bound rule is about, the derivation, is checked with that
    # function taken out: the recipe's float32 argument through an exp that is rounded once.
    arg = -(np.float32(1.0) * _spectral.distance_numpy(y[r0:r0 + m], y, metric))
    exact = np.exp(np.asarray(arg, sc.LD)).astype(np.float32)
    scale = sc.scale_of(deg_all)
    lap_exact = exact * (scale[r0:r0 + m, None] * scale[None, :])
    lap_exact[np.arange(m), r0 + np.arange(m)] = 1
    shares.update(sc.check(y, r0, m, metric, want, a=exact, lap=lap_exact, label='    with an exp rounded once'))
  if d in (2, 3) and metric != 'rbf':
    # sqrt(d2) and d1 of two or three features carry three to five roundings and the bound counts exactly those: one
    # pair in a few thousand comes within a fifth of the worst case (0.86 at d = 2 in float32 'euclidean': 2.6 u of
    # 3 u).  There the bound itself is what can be asked; the rule of one half needs roundings enough to cancel, which
    # 'rbf' has from the 4 u granted to EXP and every measure has from d = 15 on.
    del shares['A']
  assert max(shares.values()) <= 0.5, shares
  if m == n:
    assert a.tobytes() == a.T.tobytes() and lap.tobytes() == lap.T.tobytes()


@pytest.mark.parametrize('metric', sc.METRICS)
def test_the_numpy_bodies_meet_the_reference_mappers(metric):
  g = np.load(os.path.join(HERE, 'golden', 'spectral_w4.npz'))
  p, truth = sc.planted()
  assert g['points'].tobytes() == p.tobytes() and g['truth'].tobytes() == truth.tobytes()
  n, d = p.shape
  want = sc.oracle(p, metric)
  b = sc.eps(want, d, metric, np.float64)
  for r0, m in ((0, 60), (15, 15), (45, 15)):
    deg, deg_all, a, lap = _bodies(p, r0, m, metric)
    rows = slice(r0, r0 + m)
    shares = dict(
        A=sc._ratio(np.abs(a - g['A_' + metric][rows]), b['a'][rows] * want['A'][rows]),
        D=sc._ratio(np.abs(deg - g['D_' + metric][rows]), b['D'][rows] * want['D'][rows]),
        L=sc._ratio(np.abs(lap - g['L_' + metric][rows]), b['L'][rows] * want['L'][rows]))
    print('numpy %s rows %d..%d against the reference mappers: shares of the bound %s'
          % (metric, r0, r0 + m, ' '.join('%s %.3g' % kv for kv in sorted(shares.items()))))
    assert all(v <= 1.0 for v in shares.values()), shares
    assert np.all(np.diag(g['L_' + metric]) == 1) and np.all(lap[np.arange(m), r0 + np.arange(m)] == 1)
  if metric == 'rbf':           # the behaviour that is kept: the diagonal of 1 puts the leading Ritz values near 1.93
    assert np.all(np.abs(g['lanczos_d'][:3] - 1.93) < 0.01)


def test_gamma_and_empty_shapes():
  y = sc.case(20, 3, np.dtype(np.float64))
  a1 = _spectral.affinity_numpy(y[:5], y, 'rbf', 1.0)
  a2 = _spectral.affinity_numpy(y[:5], y, 'rbf', 0.5)
  assert np.allclose(a2, np.sqrt(a1), rtol=1e-14, atol=0)
  for metric in sc.METRICS:
    assert _spectral.degree_numpy(y[:0], y, metric, 1.0).shape == (0,)
    assert not np.any(_spectral.degree_numpy(y[:4], y[:0], metric, 1.0))          # n = 0: D = 0
    flat = np.zeros((4, 0))
    deg = _spectral.degree_numpy(flat, flat, metric, 1.0)                         # d = 0: every distance is 0
    assert np.all(deg == (4 if metric == 'rbf' else 0))
  one = np.ones((1, 2))
  deg = _spectral.degree_numpy(one, one, 'euclidean', 1.0)
  assert deg[0] == 0 and sc.scale_of(deg)[0] == 1
  assert _spectral.matrix_numpy(one, 0, one, 'euclidean', 1.0, scale=sc.scale_of(deg)).tolist() == [[1.0]]


def test_refusals():
  for fn in (_spectral.check_params,):
    with pytest.raises(NotImplementedError, match='np.square'):
      fn('scaled_euclidean', 1.0)
    with pytest.raises(ValueError, match='unknown metric'):
      fn('cosine', 1.0)
    for bad in (float('nan'), float('inf'), float('-inf')):
      with pytest.raises(ValueError, match='gamma'):
        fn('rbf', bad)
  assert _spectral.check_params('rbf', 2) == 2.0
