"""tests/dropout_oracle.py against published numbers: the oracle of the engine's dropout masks has to be right on its own
before tests/test_dropout_bn_gpu.py may hold the engine to it."""
import numpy as np
import pytest

from tests import dropout_oracle as do

# (counter, key) of Random123's known-answer tests for philox4x32 (kat_vectors): zeros, all ones, digits of pi
KAT_INPUTS = [
    ((0, 0, 0, 0), (0, 0)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)),
]
# their published 10-round outputs
KAT_10 = [
    (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8),
    (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD),
    (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1),
]
# 7 rounds (what the engine runs) of the same inputs, recorded from the restatement once it reproduced KAT_10
KAT_7 = [
    (0x5F6FB709, 0x0D893F64, 0x4F121F81, 0x4F730A48),
    (0x5207DDC2, 0x45165E59, 0x4D8EE751, 0x8C52F662),
    (0x4DFCCABA, 0x190A87F0, 0xC47362BA, 0xB6B5242A),
]


@pytest.mark.parametrize("rounds,expected", [(10, KAT_10), (7, KAT_7)])
def test_philox_known_answers(rounds, expected):
    for (ctr, key), exp in zip(KAT_INPUTS, expected):
        got = tuple(int(w) for w in do.philox4x32(ctr, key, rounds))
        assert got == exp, (rounds, [f"{w:08x}" for w in got])


def test_philox_is_elementwise_over_arrays():
    """the vectorised call equals the scalar call per element, and words above 2^32 are taken mod 2^32"""
    rows = np.array([0, 1, 70_000, 2 ** 32 + 1], dtype=np.uint64)[:, None]
    cols = np.arange(3, dtype=np.uint64)[None, :]
    out = do.philox4x32((rows, cols, 2, 2 ** 31 + 5), (77, 0x12345678), rounds=7)
    assert all(w.shape == (4, 3) and w.dtype == np.uint32 for w in out)
    for i, r in enumerate([0, 1, 70_000, 1]):
        for q in range(3):
            one = do.philox4x32((r, q, 2, 2 ** 31 + 5), (77, 0x12345678), rounds=7)
            assert [int(w[i, q]) for w in out] == [int(w) for w in one]


def test_threshold_and_scale_edges():
    assert do.threshold(1e-12) == 1                       # p * 2^32 < 1: clamped up, only the draw 0 is dropped
    assert do.threshold(0.5) == 2 ** 31
    assert do.threshold(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32) == 429496736   # from the float32 p, not the double 0.1
    assert do.threshold(0.999) < 2 ** 32 - 1
    assert do.threshold(1.0) == 2 ** 32 - 1               # clamped down (the engine refuses p >= 1 at creation)
    assert do.scale(0.5) == np.float32(2.0) and abs(float(do.scale(0.999)) - 1000.0) < 0.02
    assert do.scale(0.1).dtype == np.float32


def test_mask_keying():
    """every field of the documented keying moves the mask; the four words of a call land on four consecutive columns; a
    narrower or shorter mask is a corner of the wider one; the keep rate is 1 - p within 4 sigma"""
    base = dict(seed=0x1234_5678_9ABC_DEF0, rank=0, layer=1, step=3, rows=300, width=33, p=0.3)
    m = do.mask(**base)
    assert m.shape == (300, 33) and m.dtype == np.float32
    assert set(np.unique(m).tolist()) == {0.0, float(do.scale(0.3))}
    for field, other in [("seed", 0x1234_5679_9ABC_DEF0), ("seed", 0x1234_5678_9ABC_DEF1), ("rank", 3), ("layer", 0), ("step", 4),
                         ("step", 3 + 2 ** 31)]:
        assert np.mean(do.mask(**{**base, field: other}) != m) > 0.2, field
    np.testing.assert_array_equal(do.mask(**{**base, "rows": 7, "width": 5}), m[:7, :5])
    np.testing.assert_array_equal(do.mask(**{**base, "step": 3 + 2 ** 32}), m)     # the step word is taken mod 2^32
    words = do.philox4x32((11, 2, 1, 3), (0x9ABCDEF0, 0x12345678), rounds=7)
    np.testing.assert_array_equal(m[11, 8:12] != 0, np.array([int(w) >= do.threshold(0.3) for w in words]))
    keep = np.mean(m != 0)
    assert abs(keep - 0.7) < 4 * np.sqrt(0.3 * 0.7 / m.size)
    # rank r shifts key word 1 by r * 0x9E3779B9 mod 2^32
    np.testing.assert_array_equal(do.mask(**{**base, "seed": 5, "rank": 3}),
                                  do.mask(**{**base, "seed": 5 + (((3 * 0x9E3779B9) & 0xFFFFFFFF) << 32), "rank": 0}))
