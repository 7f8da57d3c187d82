"""Every consumer of csrc/kernels/philox.h against the integer oracle of
tests/philox_ref.py (pinned to the Random123 vectors by test_philox_cpu.py):
the element-wise dropout / dropout_add, the feature dropout, the Dropout2d
epilogue of the fused pool (forward and both backward kernels), the ConvNet
feature extractor and the residual dropout fused into LayerNorm. The bindings
are called directly with explicit seeds, so nothing depends on torch's
generator; only the last case (counter accounting under capture) goes through
the Python wrappers.

Masks are compared exactly. Values are compared bit for bit: one fp32 multiply
and the storage rounding, or — with a residual — one of the two correct fp32
evaluations of x·s + r (separate multiply and add, or one fused multiply-add:
the compiler may contract the expression). No bound is taken from a kernel."""
import numpy as np
import pytest
import torch

import philox_ref as R

pytestmark = pytest.mark.gpu

SEEDS = (20261019, 0x2B5C00009E3779B9)  # below 2³², and with high bits set (ops/dropout.py draws up to 2⁶²)
RATES = (0.1, 0.25, 0.5, 0.15)  # 0.15: fp32(1 / (1 - p)) differs from 1.f / (1.f - fp32(p))
F32, BF16 = torch.float32, torch.bfloat16
NAME = {F32: "f32", BF16: "bf16"}
SENTINEL = 777.0


@pytest.fixture(scope="module")
def C():
    from distributed_compute_pytorch_amd._ext import C

    return C


def bits(t):
    """The tensor's storage bits as a flat numpy array (uint32 / uint16 / uint8)."""
    t = t.detach().contiguous().reshape(-1)
    if t.dtype == F32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    if t.dtype == BF16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    assert t.dtype == torch.uint8
    return t.cpu().numpy()


def vals(t):
    """The tensor's values as flat float32 (exact for bf16)."""
    b = bits(t)
    return b.view(np.float32) if b.dtype == np.uint32 else R.bf16_to_f32(b)


def away_from_zero(rng, n):
    """float32 values with |v| in [0.5, 2] and random signs."""
    return (rng.uniform(0.5, 2.0, n) * rng.choice((-1.0, 1.0), n)).astype(np.float32)


def padded(rng, n, dtype, dev, lead):
    """(buffer, view): ``view`` = buffer[lead : lead + n], contiguous, ``lead``
    elements past the allocation's alignment, with sentinels on both sides."""
    buf = torch.full((lead + n + 5,), SENTINEL, dtype=dtype)
    buf[lead:lead + n] = torch.from_numpy(away_from_zero(rng, n)).to(dtype)
    buf = buf.to(dev)
    return buf, buf[lead:lead + n]


def check_dropout(C, dev, xd, od, n, p, seed, offset=0, offset_dev=None, res=False, xlead=0, rlead=0, rng_seed=0):
    """One _C.dropout_fwd call held to the oracle. Returns (#kept, #kept that
    match only the two-rounding form, #kept that match only the fused form)."""
    rng = np.random.default_rng(rng_seed + n)
    xbuf, x = padded(rng, n, xd, dev, xlead)
    rbuf = r = None
    if res:
        rbuf, r = padded(rng, n, od, dev, rlead)
    xb0, rb0 = xbuf.clone(), (rbuf.clone() if res else None)
    for t, lead in ((x, xlead), (r, rlead)):
        if t is not None:
            unit = 16 if t.dtype == F32 else 8
            assert (t.data_ptr() % unit == 0) == (lead * t.element_size() % unit == 0)
    off_t = None if offset_dev is None else torch.tensor([offset_dev], dtype=torch.int64, device=dev)
    y = C.dropout_fwd(x, r, p, seed, offset, None if res else od, off_t)
    torch.cuda.synchronize()
    assert y.dtype == od and tuple(y.shape) == (n,)
    # the inputs and the sentinels around them are untouched
    assert torch.equal(xbuf.view(torch.int32 if xd == F32 else torch.int16),
                       xb0.view(torch.int32 if xd == F32 else torch.int16))
    if res:
        assert torch.equal(rbuf.view(torch.int32 if od == F32 else torch.int16),
                           rb0.view(torch.int32 if od == F32 else torch.int16))
    total = (offset + (offset_dev or 0)) & R.MASK64
    keep = R.keep_elements(seed, total, n, p)
    s = R.scale(p)
    got = bits(y)
    xv = vals(x)
    if not res:
        # |x| >= 0.5: the dropped set is the exact-zero set
        bad = np.flatnonzero((got != 0) != keep)
        assert bad.size == 0, f"p={p} seed={seed:#x}: mask differs at {bad[:8]}"
        want = R.dropout_out(xv, None, keep, s, NAME[od])
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"p={p} seed={seed:#x}: values differ at {bad[:8]}"
        return int(keep.sum()), 0, 0
    rv = vals(r)
    two = R.dropout_out(xv, rv, keep, s, NAME[od])
    one = R.dropout_out(xv, rv, keep, s, NAME[od], fused=True)
    rbits = bits(r)
    assert np.array_equal(got[~keep], rbits[~keep]), "a dropped element is not the residual's bits"
    # x·s >= 0.5 in magnitude and r is a bf16/fp32 value of magnitude >= 0.5: a kept element differs from r
    assert np.all(got[keep] != rbits[keep])
    ok2, ok1 = got == two, got == one
    bad = np.flatnonzero(~(ok2 | ok1))
    assert bad.size == 0, f"p={p} seed={seed:#x}: neither fl(fl(x·s) + r) nor fl(x·s + r) at {bad[:8]}"
    return int(keep.sum()), int((ok2 & ~ok1 & keep).sum()), int((ok1 & ~ok2 & keep).sum())


# ----------------------------------------------------- a. element-wise ---
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099])
@pytest.mark.parametrize("xd,od", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)],
                         ids=["f32-f32", "f32-bf16", "bf16-f32", "bf16-bf16"])
def test_elementwise(cuda, C, xd, od, n):
    for seed in SEEDS:
        for p in RATES:
            check_dropout(C, cuda, xd, od, n, p, seed)
    # p = 1: threshold 0xFFFFFFFF, scale 0 — every element is (+)0
    x = torch.from_numpy(away_from_zero(np.random.default_rng(n), n)).to(xd).to(cuda)
    assert not bits(C.dropout_fwd(x, None, 1.0, SEEDS[0], 0, od, None)).any()


# --------------------------------------------------- b. with a residual ---
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099])
@pytest.mark.parametrize("xd,rd", [(BF16, F32), (BF16, BF16), (F32, F32), (F32, BF16)],
                         ids=["bf16+f32", "bf16+bf16", "f32+f32", "f32+bf16"])
def test_residual(cuda, C, xd, rd, n):
    kept = two = one = 0
    for seed in SEEDS:
        for p in RATES:
            k, a, b = check_dropout(C, cuda, xd, rd, n, p, seed, res=True)
            kept, two, one = kept + k, two + a, one + b
    print(f"dropout_add {NAME[xd]}+{NAME[rd]} n={n}: {kept} kept, {two} match only fl(fl(x*s)+r), "
          f"{one} match only the fused fl(x*s+r)")
    # p = 1: exactly the residual
    rng = np.random.default_rng(n)
    x = torch.from_numpy(away_from_zero(rng, n)).to(xd).to(cuda)
    r = torch.from_numpy(away_from_zero(rng, n)).to(rd).to(cuda)
    assert np.array_equal(bits(C.dropout_fwd(x, r, 1.0, SEEDS[1], 0, None, None)), bits(r))


# ------------------------------------------------------- c. scalar path ---
# A [1:] view of a fresh allocation is contiguous and misaligned: the kernel's
# vector predicate fails and every quad goes through the element loads. The
# output is allocated by the binding (aligned). fp32 (16-byte vectors) is
# misaligned at 1, 2 and 3 elements, bf16 (8-byte vectors) likewise.
MISALIGNED = [(F32, F32, 1), (F32, BF16, 1)] + [(BF16, od, o) for od in (BF16, F32) for o in (1, 2, 3)]


@pytest.mark.parametrize("which", ["x", "res", "both", "x-no-res"])
@pytest.mark.parametrize("xd,od,lead", MISALIGNED, ids=[f"{NAME[a]}-{NAME[b]}-off{o}" for a, b, o in MISALIGNED])
def test_misaligned_inputs(cuda, C, xd, od, lead, which):
    xlead = lead if which in ("x", "both", "x-no-res") else 0
    rlead = lead if which in ("res", "both") else 0
    kept = two = one = 0
    for n in (1, 3, 4, 5, 6, 7, 1023, 4099):  # n % 4 in {1, 2, 3}: the tail lanes too
        for seed, p in ((SEEDS[0], 0.1), (SEEDS[1], 0.15)):
            k, a, b = check_dropout(C, cuda, xd, od, n, p, seed, res=which != "x-no-res", xlead=xlead, rlead=rlead,
                                    rng_seed=17)
            kept, two, one = kept + k, two + a, one + b
    if which != "x-no-res":
        print(f"scalar path {NAME[xd]}+{NAME[od]} ({which} at {lead}): {kept} kept, {two} only two-rounding, "
              f"{one} only fused")


# --------------------------------------------------------- d. grid wrap ---
def test_grid_wrap(cuda, C):
    """The grid is capped at 8192 blocks x 256 threads = 2,097,152 quads: 300
    quads wrap around the grid-stride loop, and a tail of 3 follows. The whole
    mask and every value are compared (the oracle runs over 2.1 M counters)."""
    n = 4 * (8192 * 256) + 4 * 300 + 3
    seed, p = SEEDS[1], 0.1
    rng = np.random.default_rng(5)
    xv = away_from_zero(rng, n)
    y = C.dropout_fwd(torch.from_numpy(xv).to(cuda), None, p, seed, 0, None, None)
    got = bits(y)
    keep = R.keep_elements(seed, 0, n, p)
    assert got.shape == (n,)
    bad = np.flatnonzero((got != 0) != keep)
    assert bad.size == 0, f"mask differs at {bad[:8]} (first wrapped element is {4 * 8192 * 256})"
    assert np.array_equal(got, R.dropout_out(xv, None, keep, R.scale(p), "f32"))


# ----------------------------------------------------------- e. offsets ---
@pytest.mark.parametrize("offset,offset_dev,n", [
    (5, None, 23), (0, 7, 23), (5, 7, 23),  # 5 + 7: the stream of offset 12
    ((1 << 32) - 2, None, 20),  # counters 2³² - 2 … 2³² + 2: the carry into the high word
    (3, (1 << 32) - 1, 20),  # the host + device sum crosses 2³²
], ids=["host5", "dev7", "host5+dev7", "carry", "sum-crosses-2^32"])
def test_offsets(cuda, C, offset, offset_dev, n):
    for seed in SEEDS:
        for xd, od in ((F32, F32), (BF16, BF16)):
            check_dropout(C, cuda, xd, od, n, 0.25, seed, offset=offset, offset_dev=offset_dev)
            check_dropout(C, cuda, xd, od, n, 0.15, seed, offset=offset, offset_dev=offset_dev, res=True)
    if (offset, offset_dev) == (5, 7):
        x = torch.from_numpy(away_from_zero(np.random.default_rng(1), n)).to(cuda)
        both = C.dropout_fwd(x, None, 0.5, SEEDS[0], 5, None, torch.tensor([7], device=cuda))
        assert torch.equal(both, C.dropout_fwd(x, None, 0.5, SEEDS[0], 12, None, None))


# --------------------------------------------------- f. feature dropout ---
def check_feature(C, dev, shape, dtype, p, seed, offset=0, offset_dev=None):
    rows = shape[0] * shape[1]
    inner = int(np.prod(shape[2:], dtype=np.int64)) if len(shape) > 2 else 1
    rng = np.random.default_rng(rows)
    x = torch.from_numpy(away_from_zero(rng, rows * inner)).reshape(shape).to(dtype).to(dev)
    off_t = None if offset_dev is None else torch.tensor([offset_dev], dtype=torch.int64, device=dev)
    y = C.feature_dropout_fwd(x, p, seed, offset, off_t)
    assert y.dtype == dtype and y.shape == x.shape
    keep = R.keep_rows(seed, (offset + (offset_dev or 0)) & R.MASK64, rows, p)
    got = bits(y).reshape(rows, inner)
    # a plane is x · m with m = scale or 0 (a dropped negative value is -0): its magnitude bits tell the mask
    mag = got & (0x7FFFFFFF if dtype == F32 else 0x7FFF)
    assert np.array_equal((mag != 0).all(1), keep) and np.array_equal((mag == 0).all(1), ~keep), \
        f"plane mask differs at rows {np.flatnonzero((mag != 0).all(1) != keep)[:8]}"
    m = np.where(keep, R.scale(p), np.float32(0.0)).astype(np.float32)[:, None]
    want = R.store((vals(x).reshape(rows, inner) * m).astype(np.float32), NAME[dtype]).reshape(rows, inner)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5, 2, 2), (7, 9, 1, 3), (4, 8)], ids=["3x5x2x2", "7x9x1x3", "4x8"])
def test_feature_dropout(cuda, C, shape, dtype):
    for seed in SEEDS:
        for p in RATES:
            check_feature(C, cuda, shape, dtype, p, seed)
    check_feature(C, cuda, shape, dtype, 0.25, SEEDS[1], offset=5, offset_dev=7)
    check_feature(C, cuda, shape, dtype, 0.15, SEEDS[0], offset=3, offset_dev=(1 << 32) - 1)


def test_feature_dropout_block_wrap(cuda, C):
    # 66,560 rows: more than the 65,535-block grid, so 1,025 blocks take a second row
    check_feature(C, cuda, (1024, 65, 1, 1), F32, 0.1, SEEDS[1])


# ----------------------------------------------------- g. pool epilogue ---
def plane_keep(y, base):
    """(kept, dropped) per (n, c) plane of y [N, C, H, W] against the p = 0 output ``base``."""
    assert bool((base.float().abs().amax((2, 3)) > 0).all()), "a plane is all zero before dropout"
    live = (y.float().abs().amax((2, 3)) > 0).reshape(-1).cpu().numpy()
    dead = (y.float().abs().amax((2, 3)) == 0).reshape(-1).cpu().numpy()
    return live, dead


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("k,s,pad", [(2, 2, 0), (3, 2, 1)], ids=["k2s2", "k3s2p1"])  # generic / k3s2 backward kernel
@pytest.mark.parametrize("shape", [(3, 8, 4, 4), (2, 24, 5, 7)], ids=["3x8x4x4", "2x24x5x7"])
def test_pool_epilogue(cuda, C, shape, k, s, pad, dtype):
    N, Cc, H, W = shape
    rng = np.random.default_rng(N * Cc + k)
    x = torch.from_numpy(rng.normal(0.3, 1.0, shape).astype(np.float32)).to(dtype).to(cuda)
    x = x.contiguous(memory_format=torch.channels_last)
    y0, idx0 = C.maxpool2d_fwd(x, k, s, pad, True, 0.0, 0, None)
    # gy: small non-zero integers, so every window sum of the gather is exact in bf16 as in fp32
    gy = torch.from_numpy((rng.integers(1, 8, tuple(y0.shape)) * rng.choice((-1, 1), tuple(y0.shape)))
                          .astype(np.float32)).to(dtype).to(cuda).contiguous(memory_format=torch.channels_last)
    gx0 = C.maxpool2d_bwd(gy, idx0, list(shape), k, s, pad, 0.0, 0, None, None)
    for seed in SEEDS:
        for p in RATES:
            for off in (None, 7, (1 << 32) - 1):
                if off is not None and p != 0.15:
                    continue
                off_t = None if off is None else torch.tensor([off], dtype=torch.int64, device=cuda)
                keep = R.keep_rows(seed, off or 0, N * Cc, p)
                y, idx = C.maxpool2d_fwd(x, k, s, pad, True, p, seed, off_t)
                # 1. the dropped planes are the oracle's
                live, dead = plane_keep(y, y0)
                assert np.array_equal(live, keep) and np.array_equal(dead, ~keep)
                assert torch.equal(idx, idx0)
                # 2. the same stream and the same values as the feature dropout of the p = 0 output
                yf = C.feature_dropout_fwd(y0.contiguous(), p, seed, off or 0, None)
                assert np.array_equal(bits(y.contiguous()), bits(yf)), (p, seed)
                # 3. the backward scales the p = 0 gradient plane-wise: one fp32 multiply, then the storage rounding
                gx = C.maxpool2d_bwd(gy, idx, list(shape), k, s, pad, p, seed, off_t, None)
                m = np.where(keep, R.scale(p), np.float32(0.0)).astype(np.float32).reshape(N, Cc, 1, 1)
                want = R.store((vals(gx0.contiguous()).reshape(shape) * m).astype(np.float32), NAME[dtype])
                assert np.array_equal(bits(gx.contiguous()), want.reshape(-1)), (p, seed)


# ------------------------------------------------------ h. ConvNet kernel ---
@pytest.mark.parametrize("B", [5, 3])
def test_convnet_features(cuda, C, B):
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, 1, 28, 28, generator=g).to(cuda)
    w1 = (torch.randn(32, 1, 3, 3, generator=g) * 0.3).to(cuda)
    b1 = torch.full((32,), 0.1, device=cuda)
    w2 = (torch.randn(64, 32, 3, 3, generator=g) * 0.05).to(cuda)
    b2 = torch.full((64,), 1.0, device=cuda)
    out0, mask0 = C.convnet_features_fwd(x, w1, b1, w2, b2, 0.0, 0, None)
    base = vals(out0).reshape(B * 64, 144)
    assert (base > 0).any(1).all(), "a plane is all zero before dropout"
    for seed in SEEDS:
        for p in RATES:
            for off in (None, 7, (1 << 32) - 1):
                if off is not None and p != 0.15:
                    continue
                off_t = None if off is None else torch.tensor([off], dtype=torch.int64, device=cuda)
                out, mask = C.convnet_features_fwd(x, w1, b1, w2, b2, p, seed, off_t)
                keep = R.keep_rows(seed, off or 0, B * 64, p)  # row = n · 64 + c
                got = bits(out).reshape(B * 64, 144)
                assert np.array_equal((got != 0).any(1), keep), (p, seed, off)
                # kept planes: the p = 0 value times the scale — one fp32 multiply of the pooled, ReLU'd value
                # (a product cannot contract with the additions before it); dropped planes: +0
                want = (base * np.where(keep, R.scale(p), np.float32(0.0)).astype(np.float32)[:, None])
                assert np.array_equal(got, want.astype(np.float32).view(np.uint32)), (p, seed, off)
                # mask bit 2 = positive and kept; bits 0-1 (the arg-max) do not depend on the dropout
                mb, mb0 = bits(mask).reshape(B * 64, 144), bits(mask0).reshape(B * 64, 144)
                assert np.array_equal(mb & 3, mb0 & 3)
                assert np.array_equal((mb & 4) != 0, (base > 0) & keep[:, None])


# ------------------------------------ i. LayerNorm's fused residual dropout ---
# ln_forward's dispatch (layernorm.hip: vpl_for, fwd_dispatch), nv = D / 8 vectors per row:
#   D = 8, 256   ln_fwd_kernel<VPL 1, R 2, LPR 64>  (nv <= 64; D = 8: one live lane)
#   D = 768      ln_fwd_kernel<VPL 3, R 2, LPR 32>  (nv = 96: a row per half-wave)
#   D = 520      ln_fwd_kernel<VPL 2, R 2, LPR 64>  (nv = 65: the second vector on one lane only)
#   D = 1024     ln_fwd_kernel<VPL 2, R 2, LPR 64>
#   D = 1536     ln_fwd_kernel<VPL 4, R 2, LPR 64>  (nv = 192)
#   D = 4096     ln_fwd_kernel<VPL 8, R 2, LPR 64>  (nv = 512)
# each in (x, y) = (fp32, fp32), (fp32, bf16), (bf16, bf16). The backward takes the same VPL with R = 2,
# except: D = 768 runs VPL 2, and bf16 x at VPL 2 (D = 520, 768, 1024) the lean <VPL 2, R 1> kernel, which
# draws its keep bits at the store instead of with the loads.
LN_D = (8, 256, 520, 768, 1024, 1536, 4096)
LN_KINDS = [(F32, None), (F32, BF16), (BF16, None)]
LN_OFFSETS = {1: None, 5: 7, 37: (1 << 32) - 5}  # rows -> offset_dev (37 x D elements cross the carry)


@pytest.mark.parametrize("rd,yd", LN_KINDS, ids=["f32", "f32-to-bf16", "bf16"])
@pytest.mark.parametrize("D", LN_D)
def test_layer_norm_residual_dropout(cuda, C, D, rd, yd):
    kept = two = one = 0
    for rows, off in LN_OFFSETS.items():
        for seed, p in ((SEEDS[0], 0.1), (SEEDS[1], 0.15)):
            n = rows * D
            rng = np.random.default_rng(D + rows)
            branch = torch.from_numpy(away_from_zero(rng, n)).reshape(rows, D).to(BF16).to(cuda)
            res = torch.from_numpy(away_from_zero(rng, n)).reshape(rows, D).to(rd).to(cuda)
            w = torch.from_numpy(away_from_zero(rng, D)).to(cuda)
            b = torch.from_numpy(away_from_zero(rng, D)).to(cuda)
            off_t = None if off is None else torch.tensor([off], dtype=torch.int64, device=cuda)
            y, mean, rstd, xnew = C.layer_norm_fwd(res, w, b, 1e-5, yd, branch=branch, p=p, seed=seed,
                                                   offset_dev=off_t)
            assert xnew.dtype == rd and xnew.shape == res.shape
            keep = R.keep_elements(seed, off or 0, n, p)
            s = R.scale(p)
            got, rbits = bits(xnew), bits(res)
            xv, rv = vals(branch), vals(res)
            # xnew = res + dropout(branch): the oracle of the unfused dropout_add
            assert np.array_equal(got[~keep], rbits[~keep]), "a dropped element is not the residual's bits"
            assert np.all(got[keep] != rbits[keep])
            ok2 = got == R.dropout_out(xv, rv, keep, s, NAME[rd])
            ok1 = got == R.dropout_out(xv, rv, keep, s, NAME[rd], fused=True)
            bad = np.flatnonzero(~(ok2 | ok1))
            assert bad.size == 0, f"p={p} rows={rows}: neither fl(fl(x·s) + r) nor fl(x·s + r) at {bad[:8]}"
            kept, two, one = kept + int(keep.sum()), two + int((ok2 & ~ok1).sum()), one + int((ok1 & ~ok2).sum())
            # and the unfused op agrees bit for bit (same stream, same expression)
            assert np.array_equal(got, bits(C.dropout_fwd(branch, res, p, seed, 0, None, off_t)))
            # backward: the branch gradient is dx · keep · scale in bf16 — zero exactly on the dropped set
            dy = torch.from_numpy(away_from_zero(rng, n)).reshape(rows, D).to(y.dtype).to(cuda)
            dx, dw, db, gb = C.layer_norm_bwd(dy, xnew, w, b, mean, rstd, drop_p=p, drop_seed=seed,
                                              drop_offset_dev=off_t, branch_grad=True)
            assert gb.dtype == BF16 and gb.shape == res.shape
            gbits, dxv = bits(gb), vals(dx)
            assert not (gbits[~keep] & 0x7FFF).any(), "a dropped element has a branch gradient"
            # the residual gradient dx is the same value before mask and scale: a kept element is zero only where dx is
            assert np.array_equal((gbits[keep] & 0x7FFF) != 0, dxv[keep] != 0)
            assert (dxv[keep] != 0).mean() > 0.99
            if rd == F32:  # dx is stored unrounded: the branch gradient is bf16(fl32(dx · scale)) bit for bit
                want = R.f32_to_bf16(np.where(keep, dxv * s, np.float32(0.0)).astype(np.float32))
                assert np.array_equal(gbits, want)
    print(f"layer_norm D={D} {NAME[rd]}: {kept} kept, {two} match only fl(fl(x*s)+r), {one} only the fused form")


# ------------------------------------------- j. counter accounting (last) ---
def test_counter_accounting_under_capture(cuda, monkeypatch):
    """One captured graph: three ops inside batched_offsets (they read the
    device counter itself; one add at the block's end advances it past all of
    them), then two fused_dropout calls outside it (each snapshots the counter
    and advances it at once). Per replay the counter moves by the sum of
    ceil(units / 4), and every mask is the oracle's at the counter value its
    call read."""
    from distributed_compute_pytorch_amd.ops import fused_dropout, fused_feature_dropout, relu_max_pool2d_dropout
    from distributed_compute_pytorch_amd.ops import dropout as drop_mod

    seeds = []
    real = drop_mod._take_offset

    def recording(device, n):
        seed, off = real(device, n)
        seeds.append((seed, n))
        return seed, off

    monkeypatch.setattr(drop_mod, "_take_offset", recording)
    rng = np.random.default_rng(3)
    p = 0.25
    xa = torch.from_numpy(away_from_zero(rng, 10)).to(cuda)
    xf = torch.from_numpy(away_from_zero(rng, 60)).reshape(3, 5, 2, 2).to(cuda)
    xp = torch.from_numpy(rng.uniform(0.5, 2.0, (3, 8, 4, 4)).astype(np.float32)).to(cuda)
    xp = xp.contiguous(memory_format=torch.channels_last)
    xb, xc = (torch.from_numpy(away_from_zero(rng, 10)).to(cuda) for _ in range(2))

    def step():
        with drop_mod.batched_offsets():
            ya = fused_dropout(xa, p)
            yf = fused_feature_dropout(xf, p)
            yp = relu_max_pool2d_dropout(xp, 2, 2, 0, p, True)
        return ya, yf, yp, fused_dropout(xb, p), fused_dropout(xc, p)

    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st), torch.no_grad():
        step()  # eager warm-up: creates the device counter
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    counter = drop_mod._COUNTER[cuda.index]
    del seeds[:]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=st), torch.no_grad():
        ya, yf, yp, yb, yc = step()
    assert [n for _, n in seeds] == [10, 15, 24, 10, 10]
    (sa, _), (sf, _), (sp, _), (sb, _), (sc, _) = seeds
    used = [3, 4, 6, 3, 3]  # ceil(units / 4): 10 elements, 15 rows, 24 rows, 10, 10
    base_pool = torch.nn.functional.max_pool2d(xp, 2)
    for _ in range(3):
        c0 = int(counter.item())
        graph.replay()
        torch.cuda.synchronize()
        assert int(counter.item()) == c0 + sum(used)
        # batched: all three read c0
        assert np.array_equal(bits(ya) != 0, R.keep_elements(sa, c0, 10, p))
        assert np.array_equal((vals(yf).reshape(15, 4) != 0).all(1), R.keep_rows(sf, c0, 15, p))
        assert np.array_equal((vals(yf).reshape(15, 4) == 0).all(1), ~R.keep_rows(sf, c0, 15, p))
        live, dead = plane_keep(yp, base_pool)
        assert np.array_equal(live, R.keep_rows(sp, c0, 24, p)) and np.array_equal(dead, ~live)
        # unbatched: the first call reads the counter after the block's add, the second 3 further on
        assert np.array_equal(bits(yb) != 0, R.keep_elements(sb, c0 + 13, 10, p))
        assert np.array_equal(bits(yc) != 0, R.keep_elements(sc, c0 + 16, 10, p))
