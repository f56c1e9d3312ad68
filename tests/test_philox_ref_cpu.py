"""tests/philox_ref.py is sound without a GPU: the Philox block against the published known answers, and the maps'
own invariants (tests/test_random.py compares sp_random_fill with this module bit for bit)."""
import numpy as np
import pytest

from tests import philox_ref as pr

# the known-answer vectors of the Random123 distribution (kat_vectors) for philox4x32-10: counter, key, output
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
# (seed, stream position) of elements whose 53-bit uniform is >= 1 - 2^-25: float32() of it is 1.0
ROUND_TO_ONE = ((0, 8628076), (0, 24313416), (2, 16456685), (3, 8975428), (3, 23572345))


@pytest.mark.parametrize('ctr,key,want', KAT)
def test_known_answers(ctr, key, want):
  got = pr.philox4x32_10(np.array(ctr), np.array(key))
  assert got.dtype == np.uint32 and tuple(int(v) for v in got) == want


def test_known_answers_as_a_batch():
  got = pr.philox4x32_10(np.array([k[0] for k in KAT]), np.array([k[1] for k in KAT]))
  assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in KAT]


def test_counter_and_key_layout():
  # pair p of seed s is the block of counter (p lo, p hi, "SPARTAN" lo, hi) and key (s lo, s hi)
  seed, pair = 0x1234567890abcdef, (1 << 32) + 5
  got = pr.blocks(seed, pair, 3)
  for j in range(3):
    p = pair + j
    want = pr.philox4x32_10(np.array([p & 0xffffffff, p >> 32, 0x5254414e, 0x00535041]),
                            np.array([seed & 0xffffffff, seed >> 32]))
    assert np.array_equal(got[j], want)
  assert pr.CTR_HI == int.from_bytes(b'SPARTAN', 'big')
  # a seed's high word and a pair's high word both change the block
  assert not np.array_equal(pr.blocks(seed & 0xffffffff, pair, 1), got[:1])
  assert not np.array_equal(pr.blocks(seed, pair & 0xffffffff, 1), got[:1])


@pytest.mark.parametrize('seed,pos', ROUND_TO_ONE)
def test_positions_whose_uniform_rounds_to_one_in_float32(seed, pos):
  even = pos - (pos & 1)
  u = pr.uniform(seed, even, 2, np.float64)[pos - even]
  assert 1 - 2.0 ** -25 <= u < 1.0
  assert np.float32(u) == np.float32(1.0)                    # the plain cast leaves [0, 1)
  f = pr.uniform(seed, even, 2, np.float32)[pos - even]
  assert f.dtype == np.float32 and f == pr.BELOW_ONE_F32 and f < 1
  assert float(pr.BELOW_ONE_F32) == 1 - 2.0 ** -24


def test_uniform_map():
  n = 4097
  u = pr.uniform(9, 10, n)
  assert u.dtype == np.float64 and u.shape == (n,) and u.min() >= 0 and u.max() < 1
  assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53))          # 53-bit fractions
  f = pr.uniform(9, 10, n, np.float32)
  keep = u.astype(np.float32) < 1
  assert np.array_equal(f[keep], u.astype(np.float32)[keep])
  # position semantics: a fill is a window of one stream; an odd n consumes its whole last pair
  assert np.array_equal(pr.uniform(9, 10, 1001), u[:1001])
  assert np.array_equal(pr.uniform(9, 10 + 1002, 100), u[1002:1102])
  assert abs(u.mean() - 0.5) < 0.02
  with pytest.raises(AssertionError):
    pr.uniform(9, 11, 4)


def test_randint_map():
  ra, rb = pr._halves(5, 0, 6)
  for lo, hi in ((-3, 4), (0, 1), (-2**31, 0), (-2**62 + 3, 3), (-5, 2**62 - 5)):
    got = pr.randint(5, 0, 6, lo, hi)
    want = [lo + int(r) % (hi - lo) for pair in zip(ra, rb) for r in pair]
    assert got.dtype == np.int64 and [int(v) for v in got] == want
  assert pr.randint(5, 0, 6, -7, 9, np.int32).dtype == np.int32
  assert np.array_equal(pr.randint(5, 0, 6, -7, 9, np.int32), pr.randint(5, 0, 6, -7, 9))
  with pytest.raises(AssertionError):
    pr.randint(5, 0, 6, 0, 2**31 + 1, np.int32)


def test_normal_map():
  first, second, rad = pr.normal_from_uniforms(np.array([0.0, 0.0, 0.5]), np.array([0.0, 0.7, 0.25]))
  assert first[0] == 0 and second[0] == 0 and first[1] == 0 and second[1] == 0        # a == 0: exactly 0
  assert rad[0] == 0
  assert abs(float(rad[2]) - np.sqrt(2 * np.log(2.0))) < 1e-15
  assert abs(float(first[2])) < 1e-15 and abs(float(second[2] - rad[2])) < 1e-15       # angle pi / 2
  v, r = pr.normal(3, 0, 20001)
  v = np.asarray(v, np.float64)
  assert abs(v.mean()) < 0.03 and abs(v.var() - 1) < 0.05
  assert np.all(np.abs(v) <= np.asarray(r, np.float64) * (1 + 1e-15))
  assert pr.NORMAL_K == 36
