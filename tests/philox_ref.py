"""Shared by the Philox dropout tests: an integer oracle of the dropout stream,
written from the published Philox4x32-10 algorithm (Salmon, Moraes, Dror, Shaw:
"Parallel random numbers: as easy as 1, 2, 3", SC'11) in numpy, vectorised over
counters. Nothing here imports the package under test or calls a kernel;
tests/test_philox_cpu.py pins it to the Random123 known-answer vectors.

Stream. A dropout call with (seed, offset) over n units (elements, or (n, c)
rows for the feature / Dropout2d ops) uses, for unit i, word ``i % 4`` of

    philox4x32_10(key = (seed lo32, seed hi32),
                  counter = (c lo32, c hi32, 0, 0)),   c = offset + i // 4

with c a 64-bit sum (it carries into the high word and wraps at 2⁶⁴). The
unit is kept iff ``word >= threshold(p)``, threshold(p) = min(floor(fp32(p) ·
2³²), 0xFFFFFFFF); kept values are multiplied by scale(p) = fp32(1 / (1 − p)),
the quotient formed in double from the double p and rounded once.

Values. ``dropout_out`` gives the output's bits: fp32 arithmetic (numpy's
float32 operations are correctly rounded), then the storage rounding, bf16 by
round-to-nearest-even written as an integer operation.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key increments (golden ratio, sqrt(3) - 1)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
MASK64 = (1 << 64) - 1


def philox_rounds(ctr, key, rounds=10):
    """ctr: [n, 4] counter words, key: (k0, k1) — all 32-bit values. Returns uint32 [n, 4]."""
    c = np.asarray(ctr, dtype=np.uint64).reshape(-1, 4)
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0  # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _LO, n2, p0 & _LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def counters(offset, n):
    """The n consecutive 64-bit counters offset, offset + 1, … (mod 2⁶⁴) as uint64."""
    with np.errstate(over="ignore"):
        return np.uint64(int(offset) & MASK64) + np.arange(n, dtype=np.uint64)


def philox4x32_10(seed, ctrs):
    """uint32 [n, 4]: the block of every 64-bit counter in ``ctrs`` under the 64-bit ``seed``."""
    c = np.asarray(ctrs, dtype=np.uint64).reshape(-1)
    ctr = np.stack([c & _LO, c >> _S32, np.zeros_like(c), np.zeros_like(c)], axis=1)
    seed = int(seed) & MASK64
    return philox_rounds(ctr, (seed & 0xFFFFFFFF, seed >> 32))


def threshold(p):
    t = int(float(np.float32(p)) * 4294967296.0)  # fp32(p) · 2³² is exact in double
    return min(t, 0xFFFFFFFF)


def scale(p):
    return np.float32(1.0 / (1.0 - float(p))) if float(p) < 1.0 else np.float32(0.0)


def words(seed, offset, n):
    """The stream's first n uint32 words from counter ``offset`` on."""
    return philox4x32_10(seed, counters(offset, (n + 3) // 4)).reshape(-1)[:n]


def keep_elements(seed, offset, n, p):
    """bool [n]: element i is kept (word i % 4 of counter offset + i // 4 is >= threshold(p))."""
    return words(seed, offset, n) >= np.uint32(threshold(p))


def keep_rows(seed, offset, rows, p):
    """bool [rows]: the same mapping over the row indices n·C + c of a feature dropout."""
    return keep_elements(seed, offset, rows, p)


# ---------------------------------------------------------------- storage ---
def bf16_to_f32(bits):
    """uint16 bf16 patterns -> their float32 values (exact)."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16(v):
    """float32 values -> bf16 patterns, round to nearest, ties to even (NaN stays NaN)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)


def store(v, out_dtype):
    """The stored bit patterns of float32 values: uint32 for "f32", uint16 for "bf16"."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if out_dtype == "f32":
        return v.view(np.uint32).copy()
    assert out_dtype == "bf16", out_dtype
    return f32_to_bf16(v)


def dropout_out(x, res, keep, scale, out_dtype, fused=False):
    """Bits of ``res + (keep ? x · scale : 0)`` stored as ``out_dtype``.

    x, res: float32 values (bf16 inputs widened with bf16_to_f32, which is
    exact); res may be None. Without a residual a kept element is one fp32
    multiply. With one it is fl32(fl32(x·s) + r), or with ``fused=True`` the
    single-rounded fl32(x·s + r) an FMA returns. That one is formed in fp64:
    the product of two 24-bit significands is exact there, the sum is checked
    to be exact as well (it is whenever x·s and r are within a few binades of
    each other, as in the tests), so the one rounding is the conversion to
    fp32. Dropped elements are 0, or the residual unchanged."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    s = np.float32(scale)
    if res is None:
        v = np.where(keep, x * s, np.float32(0.0)).astype(np.float32)
        return store(v, out_dtype)
    r = np.ascontiguousarray(res, dtype=np.float32)
    if fused:
        prod = x.astype(np.float64) * np.float64(s)
        tot = prod + r.astype(np.float64)
        bb = tot - prod  # TwoSum: the rounding error of prod + r
        err = (prod - (tot - bb)) + (r.astype(np.float64) - bb)
        assert not np.any(err[keep] != 0.0), "x·s + r is not exact in fp64 for these inputs"
        kept = tot.astype(np.float32)
    else:
        kept = (x * s).astype(np.float32) + r
    return store(np.where(keep, kept, r).astype(np.float32), out_dtype)
