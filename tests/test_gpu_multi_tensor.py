"""The multi-tensor kernels (mt_sgd / mt_adam / mt_adadelta, mt_copy, mt_sumsq,
mt_scale_by) against the fp64 one-step oracle of tests/multi_tensor_ref.py at
the edges the older tests never reach: 16-bit parameters and state, every
flag, misaligned and partial tensors with sentinel paddings, per-tensor device
steps with an empty tensor in the list, more than 65,536 chunks, the
non-finite flag, every dtype pair of the copy and its rounding bit for bit.
Bounds: multi_tensor_ref.SLACK (NOTES §42); none is taken from the kernels."""
import math

import pytest
import torch

import multi_tensor_ref as mt

pytestmark = pytest.mark.gpu

ALL_CASES = [(k, c) for k in mt.CASES for c in mt.CASES[k]]


@pytest.fixture(scope="module")
def C():
    from distributed_compute_pytorch_amd._ext import C

    return C


def _report(what, worst):
    print(f"worst relative error beyond the storage rounding, {what}: {worst}")


# ------------------------------------------------------ a. one-step oracle ---
@pytest.mark.parametrize("dtype", mt.DTYPES, ids=mt.DTYPE_IDS)
@pytest.mark.parametrize("kind,case", ALL_CASES)
def test_one_step_oracle(cuda, C, kind, case, dtype):
    _report(f"{kind}/{case}", mt.run_case(C, kind, case, cuda, dtype))


# ----------------------------------------------- b. misalignment per list ---
# The parameters are aligned; exactly one other list sits at an element
# offset. Each kernel's vector predicate covers every list it touches (read in
# multi_tensor.hip: P, G, B / P, G, M, V, VM, SB / P, G, SQ, AC), so these take
# the scalar path; a predicate that looked at P alone would not.
MISALIGNED = [("adam", "amsgrad_decoupled_wd", mt.F32, name, 1) for name in ("g", "m", "v", "vmax")]
MISALIGNED += [("adam", "amsgrad_decoupled_wd", mt.BF16, name, off) for name in ("g", "m", "v", "vmax")
               for off in (1, 2)]
MISALIGNED += [("sgd", "nesterov_wd", mt.BF16, name, off) for name in ("g", "buf") for off in (1, 2)]


@pytest.mark.parametrize("kind,case,dtype,name,off", MISALIGNED,
                         ids=[f"{k}-{mt.DTYPE_IDS[mt.DTYPES.index(d)]}-{n}-off{o}" for k, _, d, n, o in MISALIGNED])
def test_one_misaligned_list(cuda, C, kind, case, dtype, name, off):
    offsets = {k: 0 for k in ("p", "g", "m", "v", "vmax", "buf")}
    offsets[name] = off
    _report(f"{kind}/{case} {name}@{off}", mt.run_case(C, kind, case, cuda, dtype, offsets=offsets,
                                                       layout=mt.SMALL_LAYOUT))


# ------------------------------------------- c. range updates with a shadow ---
@pytest.mark.parametrize("lo,hi", mt.RANGES)
def test_range_update_with_shadow(cuda, C, lo, hi):
    mt.run_range(C, cuda, lo, hi)


# ------------------------------------------------ d. per-tensor device steps ---
def _step_of(i):
    return mt.STEP_VALUES[i % len(mt.STEP_VALUES)]


@pytest.mark.parametrize("dtype", [mt.F32, mt.BF16], ids=["fp32", "bf16"])
def test_device_step_per_tensor(cuda, C, dtype):
    """One launch, a different device step per tensor, an empty tensor in the
    list (table index != list index)."""
    L = mt.make_lists("adam", {}, cuda, dtype)
    g = mt.make_grads({}, cuda, dtype, 0)
    steps = [torch.tensor([float(_step_of(i))], device=cuda) for i in range(len(g))]
    before = {k: [t.clone() for t in l] for k, l in L.items()}
    pads = mt.paddings(L["p"] + L["m"] + L["v"] + g)
    mt.call_kernel(C, "adam", {}, L, g, 0, steps=steps, step=7)  # the host step is not used
    worst = {k: 0.0 for k in L}
    for i in range(len(g)):
        exact = mt.one_step("ref", "adam", {}, before, g, i, 0, step=_step_of(i))
        for name, want in exact.items():
            worst[name] = max(worst[name], mt.assert_within(L[name][i], want, mt.SLACK["adam_device_step"][name],
                                                            f"step {_step_of(i)} {name}[{i}]"))
        assert float(steps[i]) == _step_of(i)
    mt.assert_paddings_intact(L["p"] + L["m"] + L["v"] + g, pads)
    _report("adam device steps", worst)


def test_host_step_at_the_same_steps(cuda, C):
    """steps=[] with step=k: the bias corrections come from the host in
    double, so the one-step slack holds at every k."""
    worst = {}
    for k in mt.STEP_VALUES:
        L = mt.make_lists("adam", {}, cuda, mt.F32)
        g = mt.make_grads({}, cuda, mt.F32, 0)
        before = {n: [t.clone() for t in l] for n, l in L.items()}
        mt.call_kernel(C, "adam", {}, L, g, 0, step=k)
        for i in range(len(g)):
            for name, want in mt.one_step("ref", "adam", {}, before, g, i, 0, step=k).items():
                worst[name] = max(worst.get(name, 0.0),
                                  mt.assert_within(L[name][i], want, mt.SLACK["adam"][name], f"step {k} {name}[{i}]"))
    _report("adam host steps", worst)


# ------------------------------------------------------------ e. grid wrap ---
NWRAP = 65600  # 3-element tensors: one chunk each, 64 more than the grid cap


def _rows(flat):
    return list(flat.view(NWRAP, 3).unbind(0))


def test_grid_wrap_sumsq(cuda, C):
    """Workgroups 0..63 own two chunks and keep a running sum. The values are
    multiples of 1/4 with Σx² < 2^24/16, so every fp32 partial sum is exact in
    any order: the result must equal the fp64 sum exactly."""
    x = ((torch.arange(3 * NWRAP, device=cuda) % 12) + 1).float() / 4
    exact = float(x.double().pow(2).sum())
    assert exact * 16 < 2 ** 24
    out = C.sumsq(_rows(x))
    assert float(out[0]) == exact and float(out[1]) == 0.0


def test_grid_wrap_adam(cuda, C):
    """An element updated twice or never is far outside the bound."""
    flat = lambda seed, **kw: mt.one_tensor(cuda, mt.F32, 3 * NWRAP, seed, **kw)  # noqa: E731
    T = {"p": flat(1), "m": flat(2, lo=0.5, hi=1.5), "v": flat(3, lo=0.5, hi=1.5, signed=False)}
    g = flat(100, lo=0.05, hi=0.25)
    before = {k: t.clone() for k, t in T.items()}
    c = mt.ADAM_DEFAULT
    C.fused_adam(_rows(T["p"]), _rows(g), _rows(T["m"]), _rows(T["v"]), [], c["lr"], c["beta1"], c["beta2"], c["eps"],
                 0.0, 2.0, False, False, False, 1.0)
    exact = dict(zip("pmv", mt.ref_adam_step(before["p"], g, before["m"], before["v"], step=2)))
    for k in "pmv":
        mt.assert_within(T[k], exact[k], mt.SLACK["adam"][k], k)


def test_grid_wrap_copy(cuda, C):
    src = mt.one_tensor(cuda, mt.F32, 3 * NWRAP, 5)
    dst = torch.zeros(3 * NWRAP, device=cuda, dtype=mt.BF16)
    C.mt_copy(_rows(src), _rows(dst), 0.5)
    mt.assert_within(dst, src.double() * 0.5, 0.0, "0.5 · x is exact in fp32: one rounding")


# ------------------------------------------------- f. sumsq and scale_by ---
@pytest.mark.parametrize("which", ["fp32", "bf16", "fp16", "mixed"])
def test_sumsq_value(cuda, C, which):
    if which == "mixed":
        xs = mt.ragged(cuda, mt.F32, 7, lo=0.05) + mt.ragged(cuda, mt.BF16, 8, lo=0.05)
    else:
        xs = mt.ragged(cuda, mt.DTYPES[mt.DTYPE_IDS.index(which)], 7, lo=0.05)
    exact = sum(float(t.double().pow(2).sum()) for t in xs)
    pads = mt.paddings(xs)
    out = C.sumsq(xs)
    rel = abs(float(out[0]) - exact) / exact
    print(f"sumsq {which}: relative error {rel:.3e}")
    assert rel <= mt.SLACK["sumsq"] and float(out[1]) == 0.0
    mt.assert_paddings_intact(xs, pads)


def test_sumsq_flag_tests_elements_not_the_sum(cuda, C):
    mt.check_sumsq_flags(C, cuda)


def test_scale_by_mixed_and_misaligned(cuda, C):
    """0.375 · x is exact in fp32 for bf16 / fp16 x and rounded once for fp32
    x: one multiply, one rounding, slack 0."""
    xs = mt.ragged(cuda, mt.F32, 7) + mt.ragged(cuda, mt.BF16, 8) + mt.ragged(cuda, mt.F16, 9, offset=3)
    before = [t.clone() for t in xs]
    pads = mt.paddings(xs)
    C.scale_by(xs, torch.tensor([0.375], device=cuda))
    for i, (t, b) in enumerate(zip(xs, before)):
        mt.assert_within(t, b.double() * 0.375, 0.0, f"tensor {i}")
    mt.assert_paddings_intact(xs, pads)


def _with_grads(dev, dtype, seed):
    gs = [t for t in mt.ragged(dev, dtype, seed, lo=0.05, hi=0.25) if t.numel() and t.dim() == 1]
    ps = [torch.zeros_like(g) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g
    return ps, gs


@pytest.mark.parametrize("dtype", [mt.F32, mt.BF16], ids=["fp32", "bf16"])
def test_clip_grad_norm_leaves_small_gradients_alone(cuda, dtype):
    """max_norm above the norm: the coefficient is exactly 1."""
    import distributed_compute_pytorch_amd as dcp

    ps, gs = _with_grads(cuda, dtype, 11)
    before = [g.clone() for g in gs]
    exact = math.sqrt(sum(float(g.double().pow(2).sum()) for g in gs))
    norm = dcp.optim.clip_grad_norm_(ps, 2.0 * exact)
    assert abs(float(norm) - exact) / exact <= mt.SLACK["sumsq"]
    for g, b in zip(gs, before):
        assert torch.equal(mt.bits(g), mt.bits(b))


def test_clip_grad_norm_bf16_above_the_threshold(cuda):
    """coef = max_norm / (norm + eps) in fp32 on the device: half the relative
    error of Σx² through the square root, plus one rounding each for the root,
    norm + eps, float(max_norm), the quotient and the product."""
    import distributed_compute_pytorch_amd as dcp

    ps, gs = _with_grads(cuda, mt.BF16, 11)
    before = [g.clone() for g in gs]
    exact = math.sqrt(sum(float(g.double().pow(2).sum()) for g in gs))
    max_norm = 0.25 * exact
    norm = dcp.optim.clip_grad_norm_(ps, max_norm)
    assert abs(float(norm) - exact) / exact <= mt.SLACK["sumsq"]
    coef = max_norm / (exact + 1e-6)
    slack = 0.5 * mt.SLACK["sumsq"] + 5 * 2.0 ** -24
    for i, (g, b) in enumerate(zip(gs, before)):
        mt.assert_within(g, b.double() * coef, slack, f"gradient {i}")


# --------------------------------------------------------------- g. mt_copy ---
@pytest.mark.parametrize("dd", mt.DTYPES, ids=mt.DTYPE_IDS)
@pytest.mark.parametrize("sd", mt.DTYPES, ids=mt.DTYPE_IDS)
def test_mt_copy_every_pair_misaligned_differently(cuda, C, sd, dd):
    scale32 = float(torch.tensor(0.37, dtype=mt.F32))
    for so, do in ((1, 0), (0, 1)):
        src = mt.ragged(cuda, sd, 21, offset=so)
        dst = mt.ragged(cuda, dd, 22, offset=do)
        src0 = [t.clone() for t in src]
        pads = mt.paddings(src + dst)
        C.mt_copy(src, dst, 0.37)
        for i, (s, d) in enumerate(zip(src, dst)):
            mt.assert_within(d, s.double() * scale32, mt.SLACK["scale"], f"src@{so} dst@{do} tensor {i}")
            assert torch.equal(mt.bits(s), mt.bits(src0[i]))
        mt.assert_paddings_intact(src + dst, pads)


_SPECIAL32 = [0x00000000, -0x80000000, 0x00000001, -0x7F800001, 0x7F800000, -0x00800000, 0x7FC00001, -0x003EDCBB,
              0x7F800001, 0x3F800000, 0x7FFF7FFF, 0x7C017E01, -0x03FF0001, 0x00017FFF]  # int32 bit patterns


@pytest.mark.parametrize("dtype", mt.DTYPES, ids=mt.DTYPE_IDS)
def test_mt_copy_same_dtype_is_bit_exact(cuda, C, dtype):
    """±0, subnormals, ±inf, quiet and signalling NaNs with payloads (as fp32
    words and as their 16-bit halves) through the raw-copy path, aligned
    (16-byte vectors + tail) and at element offset 1."""
    words = torch.tensor(_SPECIAL32, dtype=torch.int32, device=cuda).repeat(600)[:8197]
    src = words.view(dtype)
    for off in (0, 1):
        s = torch.empty(src.numel() + 8, device=cuda, dtype=dtype)[off:off + src.numel()].copy_(src)
        assert torch.equal(mt.bits(s), mt.bits(src))  # torch's copy kept the bits
        buf = torch.zeros(src.numel() + 8, device=cuda, dtype=dtype)
        d = buf[off:off + src.numel()]
        C.mt_copy([s], [d], 1.0)
        assert torch.equal(mt.bits(d), mt.bits(src))
        assert int(mt.bits(buf)[:off].abs().sum()) == 0 and int(mt.bits(buf)[off + src.numel():].abs().sum()) == 0


_ROUND_BF16 = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0x7F7FFFFF, -0x80000000, 0x007FFFFF, 0x7FC00000,
               0x7F800001, -0x00800000, 0x00008000, 0x00018000]
_ROUND_F16 = [0x3F801000, 0x3F803000, 0x3F801001, 0x3F802FFF, 0x477FF000, 0x477FEFFF, -0x80000000, 0x007FFFFF,
              0x33000000, 0x33000001, 0x33800000, 0x38FFF000, 0x7FC00000, 0x7F800001, -0x00800000, 0x7F7FFFFF]


@pytest.mark.parametrize("dd,patterns", [(mt.BF16, _ROUND_BF16), (mt.F16, _ROUND_F16)], ids=["bf16", "fp16"])
def test_mt_copy_rounds_like_torch(cuda, C, dd, patterns):
    """fp32 -> 16 bits at scale 1: exact ties with an even and an odd kept
    mantissa, their neighbours, the largest finite fp32 (rounds to inf), -0.0,
    the largest subnormal, results in the 16-bit subnormal range, NaNs, -inf.
    Bit for bit torch's conversion; NaN compared as "is NaN"."""
    src = torch.tensor(patterns, dtype=torch.int32, device=cuda).view(mt.F32)
    want = src.cpu().to(dd).to(cuda)
    for off in (0, 1):  # vector path, scalar path
        s = torch.empty(src.numel() + 4, device=cuda)[off:off + src.numel()].copy_(src)
        d = torch.zeros(src.numel() + 4, device=cuda, dtype=dd)[off:off + src.numel()]
        C.mt_copy([s], [d], 1.0)
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(d), nan)
        assert torch.equal(mt.bits(d)[~nan], mt.bits(want)[~nan]), (mt.bits(d).tolist(), mt.bits(want).tolist())
