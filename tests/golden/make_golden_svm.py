"""Records tests/golden/disdca_svm_w4.npz: the reference's own linear SVM (spartan/examples/disdca_svm.py, fit) on the
input of tests/svm_cases.golden_input -- 148 rows of 7 features, float64, labels +1 / -1 as int64 (148, 1) -- at 4
workers, T = 3, la = 0.1, with the helpers of make_golden.py (the reference tree is copied to a scratch directory,
transliterated to Python 3 there and run in process; only the arrays are kept).  divup(148, 4) = 37: the reference's
four tiles are the four chains of one tile.

  python tests/golden/make_golden_svm.py

  data, labels    the input
  alpha_1         (148, 1): the result of the first iteration's shuffle (the script watches the module's `expr.shuffle`)
  alpha_3         (148, 1): the last iteration's
  w_3             (7, 1): what fit returns
  special_alpha   (12, 1) and
  special_w       (7, 1): the reference's own _svm_disdca_train called directly on the special rows of
                  tests/svm_cases.special_case (a zero row, y = 0, both, alpha outside [0, 1] y, a row of norm 1e-200,
                  a NaN in x) with scale = 2 and lambda_n = 1.2.  The function returns alpha only; its w is kept by
                  handing it w as an ndarray subclass that remembers the results of its additions.
  whole_run       1 if the transliterated reference evaluated fit; 0 if the script had to call the reference's
                  _svm_disdca_train per band and form w in NumPy float64 (it prints what stopped it)

The script asserts that over the 444 steps each of the three branches of the clamp (at 0, inside, at 1) takes at least
a fifth of the steps, and that no step's v lies within 1e-4 of 0 or 1."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
from tests import svm_cases as case  # noqa: E402


class _Watched(object):
  """The reference's `expr` module with the results of `shuffle` kept: each one evaluated and copied where it is made.
  (In one process a fetched tile is the stored tile itself, and _svm_disdca_train writes the new alpha INTO the alpha
  it fetched: read after the run, every iteration's result shows the last one's values.)"""

  def __init__(self, real):
    self.real, self.shuffles = real, []

  def __getattr__(self, name):
    return getattr(self.real, name)

  def shuffle(self, *args, **kw):
    node = self.real.shuffle(*args, **kw)
    self.shuffles.append(np.array(node.glom(), np.float64))
    return node


class _Kept(np.ndarray):
  """A w that remembers what its additions give (the reference's loop rebinds w and returns alpha only)."""
  kept = []

  def __add__(self, other):
    out = np.add(np.asarray(self), np.asarray(other)).view(_Kept)
    _Kept.kept.append(out)
    return out


def _steps(x, y, iters, la, bands):
  """Every step's v, in NumPy float64 with plain sums (for the script's own conditions, not recorded)."""
  n, d = x.shape
  band = -(-n // bands)
  s = bands * 1.0 / (la * n)
  w, alpha, vs = np.zeros(d), np.zeros(n), []
  for _ in range(iters):
    new = alpha.copy()
    for lo in range(0, n, band):
      wb = w.copy()
      for i in range(lo, min(lo + band, n)):
        g = (y[i] - x[i].dot(wb)) / (s * x[i].dot(x[i]))
        v = y[i] * (g + alpha[i])
        vs.append(v)
        dl = y[i] * max(0, min(1, v)) - alpha[i]
        wb = wb + x[i] * s * dl
        new[i] = alpha[i] + dl
    alpha = new
    w = (x * alpha[:, None] * 1.0 / la / n).sum(axis=0)
  return np.asarray(vs)


def main():
  if not os.path.exists(os.path.join(mg.SCRATCH, 'spartan')):
    mg.prepare_tree()
    mg.build_cython()
  mg.prepare_examples()
  os.chdir(mg.SCRATCH)
  mg.install_stubs()
  sp = mg.import_reference()
  x, y = case.golden_input()
  n, d = x.shape
  workers, iters, la = case.WORKERS, case.ITERS, case.LA
  out = {'data': x, 'labels': y}

  vs = _steps(x, y.reshape(n).astype(np.float64), iters, la, workers)
  shares = [(vs <= 0).mean(), ((vs > 0) & (vs < 1)).mean(), (vs >= 1).mean()]
  nearest = min(np.abs(vs).min(), np.abs(vs - 1).min())
  print('disdca_svm_w4.npz: %d steps; clamped at 0 %.2f, inside %.2f, clamped at 1 %.2f; the nearest v to 0 or 1 is '
        '%.2g away' % (len(vs), shares[0], shares[1], shares[2], nearest))
  assert len(vs) == iters * n and min(shares) >= 0.2 and nearest > 1e-4

  from spartan.examples import disdca_svm as ref
  whole = 1
  try:
    mg.start_cluster(sp, workers)
    from spartan.config import FLAGS
    FLAGS.num_workers = workers
    ref.expr = watched = _Watched(ref.expr)
    data = sp.from_numpy(np.array(x), tile_hint=(n // workers, d))
    labels = sp.from_numpy(np.array(y), tile_hint=(n // workers, 1))
    w = ref.fit(data, labels, T=iters, la=la)
    w_3 = np.asarray(w.glom(), np.float64).reshape(d, 1)
    assert len(watched.shuffles) == iters
    alpha_1 = watched.shuffles[0].reshape(n, 1)
    alpha_3 = watched.shuffles[-1].reshape(n, 1)
    print('disdca_svm_w4.npz: fit() evaluated at %d workers' % workers)
  except Exception as e:   # noqa: BLE001  (whatever stops the transliterated reference is reported, not hidden)
    print("disdca_svm_w4.npz: the reference's fit() did not evaluate:", type(e).__name__, str(e)[:400])
    whole = 0
    band = -(-n // workers)
    w, alpha, alphas = np.zeros((d, 1)), np.zeros((n, 1)), []
    for _ in range(iters):
      new = np.empty((n, 1))
      for lo in range(0, n, band):
        hi = min(lo + band, n)
        new[lo:hi] = ref._svm_disdca_train(x[lo:hi], y[lo:hi], alpha[lo:hi].copy(), w, workers, la * n)
      alpha = new
      w = (x * alpha * 1.0 / la / n).sum(axis=0).reshape(d, 1)
      alphas.append(alpha)
    alpha_1, alpha_3, w_3 = alphas[0], alphas[-1], w

  # the special rows through the reference's own function
  sx, sy, sa, sw0, _ = case.special_case(np.float64)
  _Kept.kept = []
  with np.errstate(all='ignore'):
    special_alpha = ref._svm_disdca_train(sx, sy.reshape(-1, 1), sa.reshape(-1, 1).copy(), sw0.reshape(-1, 1).view(_Kept),
                                          case.SPECIAL_SCALE, case.SPECIAL_LAMBDA_N)
  ws = [k for k in _Kept.kept if k.shape == (sx.shape[1], 1)]
  assert len(ws) == sx.shape[0], (len(ws), [k.shape for k in _Kept.kept][:6])
  special_w = np.asarray(ws[-1], np.float64)

  # the recorded run against the script's own NumPy composition (loosely: another order of the sums)
  alphas, wn = case.run(case.yardstick, x, y)
  np.testing.assert_allclose(alpha_1.reshape(n), np.asarray(alphas[0], np.float64), rtol=0, atol=1e-9)
  np.testing.assert_allclose(alpha_3.reshape(n), np.asarray(alphas[-1], np.float64), rtol=0, atol=1e-9)
  np.testing.assert_allclose(w_3.reshape(d), np.asarray(wn, np.float64), rtol=0, atol=1e-9)
  out.update(alpha_1=alpha_1, alpha_3=alpha_3, w_3=w_3, special_alpha=np.asarray(special_alpha, np.float64),
             special_w=special_w, whole_run=np.asarray(whole, np.int64))
  path = os.path.join(HERE, 'disdca_svm_w4.npz')
  np.savez_compressed(path, **out)
  print('disdca_svm_w4.npz:', os.path.getsize(path), 'bytes;', sorted(out))


if __name__ == '__main__':
  main()
