"""sp_lda_step (csrc/lda.hip) through HipBackend.lda_step and kernels.lda_step, against the oracle and the derived
bound of tests/lda_cases.py, and the LDA driver on the HIP backend against the reference's recorded run.

Shapes (V, D, k), for the tiling that was built (include/spartan_hip_lda.h): a workgroup of the gamma kernel owns 64
documents and one of the delta kernel 64 terms, so V and D are 1 and on both sides of 64, 128 and 256; the terms pass in
chunks of 64, or of 32 (fp64, and fp32 at k > 64); a thread holds k / 16 topics rounded up to 1, 2, 4 or 8, so k is 1,
2, 16 (the last of one per thread), 33 (four per thread, 31 of 64 padded) and 128; (70, 200, 128) has four blocks of
documents for the ranges and their combine kernel.  Nothing is larger than 257 x 200 x 128.  Measured figures are printed before each
assertion (pytest -s)."""
import numpy as np
import pytest

import spartan_amd as sp
from spartan_amd import _hip, devarray, kernels
from tests import lda_cases as lc
from tests import test_lda_example as driver_case

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
SHAPES = ((1, 1, 1), (63, 64, 2), (65, 65, 16), (160, 130, 33), (257, 63, 128), (70, 200, 128))
ITERS = (1, 2, 3)
SPLITS = (0, 1, 2, 3)
ALPHA, ETA = lc.ALPHA, lc.ETA


# The driver's tests come first: they open and close contexts of their own (1 and 4 workers), which must not happen
# while the module's `be` below is open.
def test_the_tile_body_on_the_device_equals_the_reference_mappers():
  for dtype in DTYPES:
    driver_case.check_tile_body('hip', dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('workers', (1, 4))
def test_the_driver_on_the_device_equals_the_reference_run(workers, dtype):
  driver_case.check_driver('hip', workers, dtype)


def test_the_driver_on_the_device_takes_integer_counts():
  got = driver_case.check_driver('hip', 4, np.float64, as_integers=True)
  want = driver_case.check_driver('hip', 4, np.float64)
  assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.fixture(scope='module')
def be():
  ctx = sp.initialize('hip', num_workers=1)
  yield ctx.backend
  sp.shutdown()


def _framed(be, a, pad, fill=-77.0):
  """`a` as a view of a wider device array (row stride a.shape[1] + pad): (view, the whole buffer, its host image)."""
  frame = np.full((a.shape[0] + 2, a.shape[1] + pad), fill, a.dtype)
  frame[1:a.shape[0] + 1, 1:a.shape[1] + 1] = a
  buf = be.from_numpy(frame)
  return buf[1:a.shape[0] + 1, 1:a.shape[1] + 1], buf, frame


def _step(be, x, n, iters, splits=0, want_delta=True, want_doc_topics=True):
  """The outputs of one backend call on host operands, as host arrays (None for one that is not wanted)."""
  out = be.lda_step(be.from_numpy(np.ascontiguousarray(x)), be.from_numpy(np.ascontiguousarray(n)), ALPHA, ETA, iters,
                    want_delta=want_delta, want_doc_topics=want_doc_topics, splits=splits)
  return tuple(None if t is None else t.numpy() for t in out)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('iters', ITERS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_every_output_meets_the_derived_bound_at_every_split(be, shape, iters, dtype):
  v, d, k = shape
  x, n = lc.case(v, d, k, np.dtype(dtype))
  want = lc.oracle_of_case(v, d, k, np.dtype(dtype), iters)
  xt, nt = be.from_numpy(x), be.from_numpy(n)
  before = be.launches
  first = None
  for splits in SPLITS:
    out = be.lda_step(xt, nt, ALPHA, ETA, iters, splits=splits)
    delta, doc_topics = (t.numpy() for t in out)
    lc.check_step(x, n, ALPHA, ETA, iters, delta, doc_topics, want=want,
                  label='hip %s iters=%d splits=%d %s' % (shape, iters, splits, np.dtype(dtype).name))
    if first is None:
      first = (delta, doc_topics)
    assert doc_topics.tobytes() == first[1].tobytes()           # doc_topics does not depend on the ranges
    if d <= 64:
      assert delta.tobytes() == first[0].tobytes()              # one block of documents is one range whatever is asked
  assert be.launches - before == len(SPLITS)                     # (one per call: HipBackend.lda_step's docstring)
  if d > 8:
    assert np.all(np.isnan(first[1][7]))                         # the empty document
  if v > 12:
    assert not np.any(first[0][:, 11])                           # the term no document holds
  assert xt.numpy().tobytes() == x.tobytes() and nt.numpy().tobytes() == n.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_ranges_are_another_order_of_the_same_documents_and_a_repeat_gives_the_same_bits(be, dtype):
  v, d, k, iters = 70, 200, 128, 2                               # four blocks of documents
  x, n = lc.case(v, d, k, np.dtype(dtype))
  seen = {}
  for splits in (0, 1, 2, 3, 4, 9):
    delta, doc_topics = _step(be, x, n, iters, splits=splits)
    again = _step(be, x, n, iters, splits=splits)
    assert again[0].tobytes() == delta.tobytes() and again[1].tobytes() == doc_topics.tobytes()
    seen[splits] = delta.tobytes()
  assert seen[9] == seen[4] == seen[0]          # min(s, 4) ranges; the library's choice here: every block a range
  assert len({seen[1], seen[2], seen[3], seen[4]}) == 4


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('iters', (1, 3))
def test_a_document_depends_on_itself_and_the_counts_alone(be, iters, dtype):
  v, d, k = 70, 131, 33
  x, n = lc.case(v, d, k, np.dtype(dtype), seed=2)
  delta, doc_topics = _step(be, x, n, iters)
  for i in (0, 7, 63, 64, 130):                                   # alone: another place in the workgroup, no neighbours
    _, alone = _step(be, x[:, i:i + 1], n, iters)
    assert alone.tobytes() == doc_topics[i:i + 1].tobytes(), i
  _, shifted = _step(be, x[:, 1:], n, iters)                      # the band of documents shifted by one
  assert shifted.tobytes() == doc_topics[1:].tobytes()
  changed = np.array(x)
  changed[:, 4] = changed[::-1, 4] + 1
  dc, tc = _step(be, changed, n, iters)
  assert np.delete(tc, 4, axis=0).tobytes() == np.delete(doc_topics, 4, axis=0).tobytes()
  assert tc[4].tobytes() != doc_topics[4].tobytes() and dc.tobytes() != delta.tobytes()
  # an empty document adds exactly nothing: without it, the same delta bit for bit (the documents before it are
  # added in the same order; 7 is in the first block, so take a single range)
  d1, _ = _step(be, x, n, iters, splits=1)
  moved = np.concatenate([np.delete(x, 7, axis=1), x[:, 7:8]], axis=1)          # the empty document last
  d2, t2 = _step(be, moved, n, iters, splits=1)
  assert np.all(np.isnan(t2[-1])) and t2[:-1].tobytes() == np.delete(doc_topics, 7, axis=0).tobytes()
  lc.check_step(moved, n, ALPHA, ETA, iters, d2, t2, label='hip empty document last')
  assert np.all(np.isfinite(d1)) and d1.tobytes() == d2.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_signed_counts(be, dtype):
  v, d, k, iters = 70, 130, 33, 2
  x, n = lc.case(v, d, k, np.dtype(dtype), signed=True)
  delta, doc_topics = _step(be, x, n, iters)
  lc.check_step(x, n, ALPHA, ETA, iters, delta, doc_topics, want=lc.oracle_of_case(v, d, k, np.dtype(dtype), iters, signed=True),
                label='hip signed counts %s' % np.dtype(dtype).name)
  of_abs = _step(be, np.abs(x), n, iters)
  assert of_abs[1].tobytes() == doc_topics.tobytes()              # |x| in c
  assert np.all(delta <= of_abs[0]) and np.any(delta < of_abs[0])  # the signed x in delta


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('shape', ((70, 131, 33), (65, 5, 128)), ids=lambda s: '%dx%dx%d' % s)
def test_views_of_wider_buffers_and_null_outputs_give_the_same_bits(be, shape, dtype):
  v, d, k = shape
  iters = 2
  x, n = lc.case(v, d, k, np.dtype(dtype), seed=1)
  delta, doc_topics = _step(be, x, n, iters)
  (xt, xbuf, xframe), (nt, nbuf, nframe) = _framed(be, x, 3), _framed(be, n, 5)
  (dt_, dbuf, dframe), (tt, tbuf, tframe) = _framed(be, np.zeros((k, v), dtype), 7), _framed(be, np.zeros((d, k), dtype), 2)
  kernels.lda_step(xt, nt, ALPHA, ETA, iters, delta=dt_, doc_topics=tt)
  assert dt_.numpy().tobytes() == delta.tobytes() and tt.numpy().tobytes() == doc_topics.tobytes()
  assert xbuf.numpy().tobytes() == xframe.tobytes() and nbuf.numpy().tobytes() == nframe.tobytes()
  dframe[1:k + 1, 1:v + 1] = delta
  tframe[1:d + 1, 1:k + 1] = doc_topics
  assert dbuf.numpy().tobytes() == dframe.tobytes()                # frames untouched
  assert np.array_equal(tbuf.numpy(), tframe, equal_nan=True)
  # the backend takes the views too (a column band of a wider matrix is what the driver's tiles are)
  out = be.lda_step(xt, nt, ALPHA, ETA, iters)
  assert out[0].numpy().tobytes() == delta.tobytes() and out[1].numpy().tobytes() == doc_topics.tobytes()
  # each output alone
  only_delta = _step(be, x, n, iters, want_doc_topics=False)
  only_topics = _step(be, x, n, iters, want_delta=False)
  assert only_delta[1] is None and only_delta[0].tobytes() == delta.tobytes()
  assert only_topics[0] is None and only_topics[1].tobytes() == doc_topics.tobytes()
  d2 = be.empty((k, v), dtype)
  kernels.lda_step(xt, nt, ALPHA, ETA, iters, delta=d2)
  t2 = be.empty((d, k), dtype)
  kernels.lda_step(xt, nt, ALPHA, ETA, iters, doc_topics=t2)
  assert d2.numpy().tobytes() == delta.tobytes() and t2.numpy().tobytes() == doc_topics.tobytes()


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: np.dtype(d).name)
def test_no_document_and_no_term(be, dtype):
  n = lc.case(6, 1, 4, np.dtype(dtype))[1]
  delta, doc_topics = _step(be, np.zeros((6, 0), dtype), n, 2)
  assert delta.shape == (4, 6) and doc_topics.shape == (0, 4) and not np.any(delta)
  delta, doc_topics = _step(be, np.zeros((0, 66), dtype), np.zeros((4, 0), dtype), 2)
  assert delta.shape == (4, 0) and doc_topics.shape == (66, 4) and np.all(np.isnan(doc_topics))
  delta, doc_topics = _step(be, np.zeros((6, 3), dtype), n, 3)                    # every document empty
  assert not np.any(delta) and np.all(np.isnan(doc_topics))


def test_refusals_launch_nothing_and_leave_the_outputs_untouched(be):
  x, n = lc.case(9, 5, 4, np.dtype(np.float32))
  xt, nt = be.from_numpy(x), be.from_numpy(n)
  before = be.launches
  for bad_x, bad_n in ((x.astype(np.int32), n.astype(np.int32)), (x.astype(np.float16), n.astype(np.float16)),
                       (x, n.astype(np.float64)), (x.astype(np.int32), n)):
    with pytest.raises(TypeError, match='astype'):
      be.lda_step(be.from_numpy(bad_x), be.from_numpy(bad_n), ALPHA, ETA, 1)
  for bad in (0.0, -1.0, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='alpha = '):
      be.lda_step(xt, nt, bad, ETA, 1)
    with pytest.raises(ValueError, match='eta = '):
      be.lda_step(xt, nt, ALPHA, bad, 1)
  with pytest.raises(ValueError, match='iters = 0'):
    be.lda_step(xt, nt, ALPHA, ETA, 0)
  with pytest.raises(ValueError, match='k = 0'):
    be.lda_step(xt, be.from_numpy(np.zeros((0, 9), np.float32)), ALPHA, ETA, 1)
  with pytest.raises(ValueError, match='k = 129'):
    be.lda_step(xt, be.from_numpy(np.ones((129, 9), np.float32)), ALPHA, ETA, 1)
  with pytest.raises(ValueError, match='fit'):
    be.lda_step(xt, be.from_numpy(np.zeros((4, 8), np.float32)), ALPHA, ETA, 1)
  delta, doc_topics = be.from_numpy(np.full((4, 9), -5.0, np.float32)), be.from_numpy(np.full((5, 4), -6.0, np.float32))
  with pytest.raises(TypeError, match='astype'):
    kernels.lda_step(xt, be.from_numpy(n.astype(np.float64)), ALPHA, ETA, 1, delta=delta, doc_topics=doc_topics)
  with pytest.raises(TypeError, match='astype'):
    kernels.lda_step(xt, nt, ALPHA, ETA, 1, delta=be.empty((4, 9), np.float64))
  with pytest.raises(ValueError, match='alpha = '):
    kernels.lda_step(xt, nt, 0.0, ETA, 1, delta=delta, doc_topics=doc_topics)
  with pytest.raises(ValueError, match='splits'):
    kernels.lda_step(xt, nt, ALPHA, ETA, 1, delta=delta, doc_topics=doc_topics, splits=-1)
  for bad in (dict(delta=be.empty((4, 8), np.float32)), dict(doc_topics=be.empty((5, 5), np.float32)),
              dict(delta=be.empty((9, 4), np.float32))):
    with pytest.raises(ValueError, match='targets'):
      kernels.lda_step(xt, nt, ALPHA, ETA, 1, **bad)
  assert be.launches == before
  # the library's own refusals: a code and a message each, the outputs as they were
  import ctypes as C
  lib, err = _hip.extras(), _hip.lib().sp_last_error
  f32 = _hip.SP_F32
  ws = devarray.empty((lib.sp_lda_step_workspace_bytes(f32, 9, 5, 4, 1, 0),), np.uint8)
  px, pn, pd, pt, pw = (C.c_void_p(t.data_ptr()) for t in (xt, nt, delta, doc_topics, ws))

  def call(dtype=f32, ldx=5, v=9, d=5, ldn=9, k=4, alpha=ALPHA, eta=ETA, iters=1, splits=0, ldd=9, ldt=4, wsb=None):
    return lib.sp_lda_step(dtype, px, ldx, v, d, pn, ldn, k, alpha, eta, iters, splits, pd, ldd, pt, ldt, pw,
                           ws.numel() if wsb is None else wsb, kernels._stream())

  for kw, word in ((dict(dtype=_hip.SP_I32), 'astype'), (dict(dtype=_hip.SP_F16), 'astype'), (dict(k=0), 'k = 0'),
                   (dict(k=129), 'k = 129'), (dict(iters=0), 'iters = 0'), (dict(alpha=0.0), 'alpha = '),
                   (dict(alpha=float('nan')), 'alpha = '), (dict(alpha=float('inf')), 'alpha = '), (dict(eta=0.0), 'eta = '),
                   (dict(eta=-0.5), 'eta = '), (dict(eta=float('nan')), 'eta = '), (dict(eta=float('inf')), 'eta = '),
                   (dict(ldx=4), 'bad shape'), (dict(ldn=8), 'bad shape'), (dict(ldd=8), 'bad shape'), (dict(ldt=3), 'bad shape'),
                   (dict(splits=-1), 'bad shape'), (dict(v=-1), 'bad shape'), (dict(d=-1), 'bad shape'), (dict(wsb=16), 'workspace')):
    assert call(**kw) != 0, kw
    assert word in err().decode(), (kw, err().decode())
  be.synchronize()
  assert np.all(delta.numpy() == -5.0) and np.all(doc_topics.numpy() == -6.0)
  assert call() == 0                                                # (the same arguments, none of them bad, are taken)
  be.synchronize()
  got = _step(be, x, n, 1)
  assert delta.numpy().tobytes() == got[0].tobytes() and doc_topics.numpy().tobytes() == got[1].tobytes()
