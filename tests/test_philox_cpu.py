"""Pins the Philox dropout oracle (tests/philox_ref.py) to facts outside this
project: the Random123 known-answer vectors of philox4x32-10, hand-computed
thresholds, and the counter mapping's algebra. The GPU tests
(test_gpu_philox_dropout.py) then hold every kernel to the oracle."""
import numpy as np
import pytest

import philox_ref as R

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, expected)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answer_vectors(ctr, key, want):
    got = R.philox_rounds(np.array([ctr], dtype=np.uint64), key)
    assert got.dtype == np.uint32 and got.shape == (1, 4)
    assert tuple(int(v) for v in got[0]) == want


def test_vectorised_and_public_entry_agree_with_round_function():
    # many counters at once == one at a time, and the public entry point is
    # the round function on (lo32, hi32, 0, 0) with key (seed lo32, seed hi32)
    seed = 0x299F31D0A4093822
    ctrs = np.array([0, 1, 0xFFFFFFFF, 0x100000000, 0x85A308D3243F6A88, R.MASK64], dtype=np.uint64)
    got = R.philox4x32_10(seed, ctrs)
    for row, c in zip(got, ctrs):
        c = int(c)
        one = R.philox_rounds([[c & 0xFFFFFFFF, c >> 32, 0, 0]], (0xA4093822, 0x299F31D0))
        assert np.array_equal(row, one[0])
    # the first known-answer vector is reachable through the public entry point
    assert tuple(int(v) for v in R.philox4x32_10(0, [0])[0]) == KAT[0][2]


def test_threshold_values():
    assert R.threshold(0.25) == 1 << 30
    assert R.threshold(0.5) == 1 << 31
    assert R.threshold(1.0) == 0xFFFFFFFF
    # fp32(0.1) = 13421773 · 2⁻²⁷, so fp32(0.1) · 2³² = 13421773 · 32, an integer
    assert R.threshold(0.1) == 13421773 * 32 == 429496736
    assert R.threshold(0.0) == 0


def test_scale_is_the_correctly_rounded_quotient():
    from fractions import Fraction

    for pct in range(1, 100):
        p = pct / 100.0
        s = R.scale(p)
        exact = 1 / (1 - Fraction(p))
        # nearest fp32: no neighbour is closer
        for nb in (np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(4e9))):
            assert abs(Fraction(float(s)) - exact) <= abs(Fraction(float(nb)) - exact), p
    assert R.scale(1.0) == 0.0
    # the rate at which the fp32 formula 1.f / (1.f - fp32(p)) is one ulp off
    assert R.scale(0.15) != np.float32(1.0) / (np.float32(1.0) - np.float32(0.15))
    assert R.scale(0.15).view(np.uint32) == np.float32(1.17647064).view(np.uint32)


@pytest.mark.parametrize("seed", [20261019, 0x3A5C_0000_9E37_79B9])
@pytest.mark.parametrize("off", [0, 1, 5, (1 << 32) - 2])
def test_counter_mapping(seed, off):
    p, n = 0.3, 23
    if off < 100:
        whole = R.keep_elements(seed, 0, n + 4 * off, p)
        assert np.array_equal(R.keep_elements(seed, off, n, p), whole[4 * off:])
    assert np.array_equal(R.keep_rows(seed, off, n, p), R.keep_elements(seed, off, n, p))
    # element i is word i % 4 of counter off + i // 4
    w = R.words(seed, off, n)
    for i in (0, 3, 4, 9, 22):
        blk = R.philox4x32_10(seed, [(off + i // 4) & R.MASK64])[0]
        assert int(w[i]) == int(blk[i % 4])
    # a prefix does not depend on n
    assert np.array_equal(R.keep_elements(seed, off, 7, p), R.keep_elements(seed, off, n, p)[:7])


def test_carry_into_the_high_counter_word():
    c = R.counters((1 << 32) - 2, 5)
    assert [int(v) >> 32 for v in c] == [0, 0, 1, 1, 1]
    assert [int(v) & 0xFFFFFFFF for v in c] == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1, 2]
    seed = 0x1234_5678_9ABC_DEF0
    right = R.philox4x32_10(seed, c)
    dropped = R.philox4x32_10(seed, c & np.uint64(0xFFFFFFFF))
    assert np.array_equal(right[:2], dropped[:2])
    assert not np.array_equal(right[2:], dropped[2:])
    for i in range(2, 5):  # every block past the carry differs in every word
        assert not np.any(right[i] == dropped[i])
    # the counter wraps at 2⁶⁴
    assert [int(v) for v in R.counters(R.MASK64, 2)] == [R.MASK64, 0]


def test_bf16_rounding_ties_to_even():
    f = lambda *bits: np.array(bits, dtype=np.uint32).view(np.float32)
    got = R.f32_to_bf16(f(0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0x7F7FFFFF))
    assert [int(v) for v in got] == [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0xBF80, 0x7F80]
    back = R.bf16_to_f32(np.array([0x3F80, 0xC000], dtype=np.uint16))
    assert [float(v) for v in back] == [1.0, -2.0]


def test_dropout_out_forms():
    x = np.array([1.5, -0.75, 1.0000001, 0.5], dtype=np.float32)
    r = np.array([0.25, 2.0, -1.0, 3.0], dtype=np.float32)
    keep = np.array([True, False, True, True])
    s = R.scale(0.15)
    out = R.dropout_out(x, None, keep, s, "f32").view(np.float32)
    assert out[1] == 0.0 and out[0] == np.float32(1.5) * s
    two = R.dropout_out(x, r, keep, s, "f32").view(np.float32)
    one = R.dropout_out(x, r, keep, s, "f32", fused=True).view(np.float32)
    assert two[1] == one[1] == np.float32(2.0)  # dropped: the residual itself
    # the two evaluations are within one fp32 ulp of each other, and the fused
    # one is the rounding of the exact value
    from fractions import Fraction

    for i in (0, 2, 3):
        exact = Fraction(float(x[i])) * Fraction(float(s)) + Fraction(float(r[i]))
        assert abs(Fraction(float(one[i])) - exact) <= abs(Fraction(float(two[i])) - exact)
        assert abs(int(one.view(np.uint32)[i]) - int(two.view(np.uint32)[i])) <= 1
    assert R.dropout_out(x, r, keep, s, "bf16").dtype == np.uint16
