"""RMSNorm, rotary embedding and SwiGLU kernels (csrc/kernels/rmsnorm.hip,
rope.hip, swiglu.hip) against fp64 references computed from the same bf16 /
fp32 inputs, their capture / replay behaviour, and the Llama model on them
against the plain-PyTorch variant.

Tolerances are those of the LayerNorm and GELU cases of
test_gpu_transformer_ops.py (the arithmetic is the same: fp32 row statistics,
one rounding to bf16): y / dx rtol 1e-4, atol 1e-4 (fp32), rtol 2e-2, atol
3e-2 (bf16); dγ rtol 1e-3, atol 1e-3·√rows (fp32), 0.05·√rows (bf16); SwiGLU
forward rtol 1e-2, atol 1e-2, backward rtol 1e-2, atol 2e-2. RoPE is held to
one bf16 ulp of the fp64 result rounded to bf16.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _rms_ref64(x, w, g, eps, extra=None):
    """fp64 (y, dx, dw) of RMSNorm from the given inputs; extra: a second gradient of x."""
    xd, wd, gd = x.double(), w.double(), g.double()
    D = x.shape[-1]
    rstd = torch.rsqrt((xd * xd).mean(-1, keepdim=True) + eps)
    y = xd * rstd * wd
    gw = gd * wd
    dx = rstd * gw - xd * rstd ** 3 * (gw * xd).sum(-1, keepdim=True) / D
    if extra is not None:
        dx = dx + extra.double()
    dw = (gd * xd * rstd).reshape(-1, D).sum(0)
    return y, dx, dw


def _rms_tols(dtype, rows):
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=2e-2, atol=3e-2)
    watol = 1e-3 * rows ** 0.5 if dtype == torch.float32 else 0.05 * rows ** 0.5
    return tol, dict(rtol=1e-3, atol=watol)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("D", [8, 72, 768, 1024, 4096])
@pytest.mark.parametrize("rows", [1, 3, 127, 4097])
def test_rms_norm_matches_fp64(cuda, dtype, D, rows):
    from distributed_compute_pytorch_amd.ops import fused_rms_norm

    torch.manual_seed(0)
    eps = 1e-6
    x = (torch.randn(rows, D, device=cuda) * 3 + 1).to(dtype)
    w = (torch.rand(D, device=cuda) + 0.5).requires_grad_()
    g = torch.randn(rows, D, device=cuda).to(dtype)
    yr, dxr, dwr = _rms_ref64(x, w.detach(), g, eps)
    xo = x.clone().requires_grad_()
    y = fused_rms_norm(xo, w, eps)
    assert y.dtype == dtype
    y.backward(g)
    tol, wtol = _rms_tols(dtype, rows)
    torch.testing.assert_close(y.double(), yr, **tol)
    torch.testing.assert_close(xo.grad.double(), dxr, **tol)
    torch.testing.assert_close(w.grad.double(), dwr, **wtol)
    # no float atomics: a second call gives the same bits
    y1, dx1, dw1 = y.detach().clone(), xo.grad.clone(), w.grad.clone()
    xo.grad = w.grad = None
    fused_rms_norm(xo, w, eps).backward(g)
    assert torch.equal(fused_rms_norm(xo, w, eps).detach(), y1)
    assert torch.equal(xo.grad, dx1) and torch.equal(w.grad, dw1)


def test_rms_norm_autocast_fp32_in_bf16_out(cuda):
    """The autocast residual stream: fp32 x, bf16 y, bf16 dy, fp32 dx."""
    from distributed_compute_pytorch_amd.ops import FusedRMSNorm

    torch.manual_seed(0)
    rows, D = 257, 768
    m = FusedRMSNorm(D).to(cuda)
    with torch.no_grad():
        m.weight.copy_(torch.rand(D, device=cuda) + 0.5)
    x = (torch.randn(rows, D, device=cuda) * 3 + 1).requires_grad_()
    g = torch.randn(rows, D, device=cuda).to(BF)
    with torch.autocast("cuda", dtype=BF):
        y = m(x)
    assert y.dtype == BF
    y.backward(g)
    assert x.grad.dtype == torch.float32
    yr, dxr, dwr = _rms_ref64(x.detach(), m.weight.detach(), g, m.eps)
    tol, wtol = _rms_tols(BF, rows)
    torch.testing.assert_close(y.double(), yr, **tol)
    torch.testing.assert_close(x.grad.double(), dxr, **tol)
    torch.testing.assert_close(m.weight.grad.double(), dwr, **wtol)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,D", [(131, 768), (37, 4096), (5, 72)])
def test_rms_norm_dual_sums_both_gradients(cuda, dtype, rows, D):
    """forward_dual: the alias's gradient is added into dx inside the kernel."""
    from distributed_compute_pytorch_amd.ops import FusedRMSNorm

    torch.manual_seed(0)
    m = FusedRMSNorm(D).to(cuda)
    with torch.no_grad():
        m.weight.copy_(torch.rand(D, device=cuda) + 0.5)
    x = (torch.randn(rows, D, device=cuda) * 3 + 1).to(dtype).requires_grad_()
    g = torch.randn(rows, D, device=cuda).to(dtype)
    g2 = torch.randn(rows, D, device=cuda).to(dtype)
    y, alias = m.forward_dual(x)
    assert alias.data_ptr() == x.data_ptr()
    torch.autograd.backward([y, alias], [g, g2])
    yr, dxr, dwr = _rms_ref64(x.detach(), m.weight.detach(), g, m.eps, extra=g2)
    tol, wtol = _rms_tols(dtype, rows)
    torch.testing.assert_close(y.double(), yr, **tol)
    torch.testing.assert_close(x.grad.double(), dxr, **tol)
    torch.testing.assert_close(m.weight.grad.double(), dwr, **wtol)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_rms_norm_in_place_accumulation(cuda, dtype):
    """Under accumulate_grads_in_place dγ is added into the existing fp32 .grad."""
    from distributed_compute_pytorch_amd.ops import FusedRMSNorm
    from distributed_compute_pytorch_amd.ops.linear import accumulate_grads_in_place

    torch.manual_seed(0)
    rows, D = 300, 768
    a = FusedRMSNorm(D).to(cuda)
    with torch.no_grad():
        a.weight.copy_(torch.rand(D, device=cuda) + 0.5)
    xs = [(torch.randn(rows, D, device=cuda) * 3 + 1).to(dtype) for _ in range(2)]
    gs = [torch.randn(rows, D, device=cuda).to(dtype) for _ in range(2)]
    a(xs[0]).backward(gs[0])
    first = a.weight.grad
    ptr, g0 = first.data_ptr(), first.clone()
    with accumulate_grads_in_place():
        a(xs[1]).backward(gs[1])
    assert a.weight.grad.data_ptr() == ptr
    a2 = copy.deepcopy(a)
    a2.weight.grad = None
    a2(xs[1]).backward(gs[1])
    torch.testing.assert_close(a.weight.grad, g0 + a2.weight.grad, rtol=1e-6, atol=1e-6 * float(g0.abs().max()))
    dwr = sum(_rms_ref64(x, a.weight.detach(), g, a.eps)[2] for x, g in zip(xs, gs))
    _, wtol = _rms_tols(dtype, 2 * rows)
    torch.testing.assert_close(a.weight.grad.double(), dwr, **wtol)


def test_rms_norm_unsupported_width_falls_back(cuda):
    from distributed_compute_pytorch_amd._ext import C as _C
    from distributed_compute_pytorch_amd.ops import fused_rms_norm

    assert not _C.rms_norm_supported(4104) and not _C.rms_norm_supported(12) and _C.rms_norm_supported(4096)
    torch.manual_seed(0)
    rows, D = 9, 4104
    x = (torch.randn(rows, D, device=cuda) * 3 + 1).to(BF).requires_grad_()
    w = (torch.rand(D, device=cuda) + 0.5).requires_grad_()
    g = torch.randn(rows, D, device=cuda).to(BF)
    y = fused_rms_norm(x, w, 1e-6)
    y.backward(g)
    yr, dxr, dwr = _rms_ref64(x.detach(), w.detach(), g, 1e-6)
    tol, wtol = _rms_tols(BF, rows)
    torch.testing.assert_close(y.double(), yr, **tol)
    torch.testing.assert_close(x.grad.double(), dxr, **tol)
    torch.testing.assert_close(w.grad.double(), dwr, **wtol)


# ------------------------------------------------------------------ RoPE ---
def _rope_ref64(qkv, heads, table, inverse=False):
    B, T, _ = qkv.shape
    cos = table[:T, 0].double()[None, :, None, :]
    sin = table[:T, 1].double()[None, :, None, :] * (-1.0 if inverse else 1.0)
    qk = qkv[..., :2 * heads * 64].double().reshape(B, T, 2 * heads, 64)
    a, b = qk[..., :32], qk[..., 32:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], -1).reshape(B, T, 2 * heads * 64)


def _bf16_key(t):
    """bf16 values as integers in value order: neighbours differ by 1 (±0 -> 0)."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def _bf16_from_key(k):
    return torch.where(k >= 0, k, -k - 32768).to(torch.int16).view(BF)


def _assert_within_one_bf16_ulp(got, ref64):
    """got (bf16) is the fp64 value rounded to bf16, or a neighbour of it. The
    rounding is done here in one step: fp64 -> fp32 -> bf16 rounds twice and
    lands a whole ulp off when the fp32 step hits a bf16 midpoint. Compared on
    the ordered bit patterns, so no ulp is computed in floating point."""
    k0 = _bf16_key(ref64.float().to(BF))
    cands = torch.stack([k0 - 1, k0, k0 + 1])
    err = (_bf16_from_key(cands).double() - ref64.unsqueeze(0)).abs()
    kr = cands.gather(0, err.argmin(0, keepdim=True))[0]
    d = (_bf16_key(got) - kr).abs()
    if int(d.max()) > 1:
        i = int(d.reshape(-1).argmax())
        raise AssertionError(f"{int((d > 1).sum())} elements off by more than one bf16 ulp; worst: got "
                             f"{float(got.reshape(-1)[i])!r}, fp64 {float(ref64.reshape(-1)[i])!r} "
                             f"({int(d.reshape(-1)[i])} ulps)")


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("heads", [1, 12])
@pytest.mark.parametrize("T", [64, 192])
def test_rope_matches_fp64(cuda, T, heads, inplace):
    from distributed_compute_pytorch_amd.ops import apply_rope_qkv, rope_table
    from distributed_compute_pytorch_amd.ops.rope import rope_qkv_reference

    torch.manual_seed(0)
    B, C = 2, heads * 64
    table = rope_table(256, 10000.0, cuda)
    qkv = (torch.randn(B, T, 3 * C, device=cuda) * 2).to(BF)
    src = qkv.clone()
    ref = _rope_ref64(src, heads, table)
    y = apply_rope_qkv(qkv, heads, table, inplace=inplace)
    assert (y.data_ptr() == qkv.data_ptr()) == inplace
    if not inplace:
        assert torch.equal(qkv, src)
    _assert_within_one_bf16_ulp(y[..., :2 * C], ref)
    assert torch.equal(y[..., 2 * C:], src[..., 2 * C:])  # v: the input's bits
    # backward: against autograd through the PyTorch path, and the fp64 inverse rotation
    g = torch.randn(B, T, 3 * C, device=cuda).to(BF)
    a = src.clone().requires_grad_()
    (apply_rope_qkv(a * 1, heads, table, inplace=inplace).float() * g.float()).sum().backward()
    b = src.clone().requires_grad_()
    (rope_qkv_reference(b, heads, table).float() * g.float()).sum().backward()
    _assert_within_one_bf16_ulp(a.grad[..., :2 * C], _rope_ref64(g, heads, table, inverse=True))
    _assert_within_one_bf16_ulp(a.grad[..., :2 * C], b.grad[..., :2 * C].double())
    assert torch.equal(a.grad[..., 2 * C:], g[..., 2 * C:]) and torch.equal(b.grad[..., 2 * C:], g[..., 2 * C:])


def test_rope_row_t_uses_table_row_t(cuda):
    from distributed_compute_pytorch_amd.ops import apply_rope_qkv, rope_table

    heads, T, t0 = 2, 128, 37
    C = heads * 64
    table = rope_table(256, 10000.0, cuda)
    qkv = torch.zeros(2, T, 3 * C, device=cuda, dtype=BF)
    qkv[1, t0] = 1.0
    y = apply_rope_qkv(qkv, heads, table)
    cos, sin = table[t0, 0].double(), table[t0, 1].double()
    want = torch.cat([cos - sin, cos + sin]).repeat(2 * heads)
    _assert_within_one_bf16_ulp(y[1, t0, :2 * C], want)
    assert torch.equal(y[1, t0, 2 * C:], qkv[1, t0, 2 * C:])
    y[1, t0] = 0
    assert not bool(y.any())  # every other position stays exactly zero
    with pytest.raises(ValueError):
        apply_rope_qkv(torch.zeros(1, 320, 3 * C, device=cuda, dtype=BF), heads, table)


def test_rope_in_place_leaves_the_linear_backward_intact(cuda):
    """packed_linear -> rope (in place on the GEMM output) -> weighted sum: the
    Linear's input, weight and bias gradients equal those of the out-of-place
    kernel (same kernels' bits up to the GEMMs' own order) and of the
    out-of-place PyTorch path. Bound for the latter: the two rope backwards
    differ by at most one bf16 ulp (2^-8 relative) per element of the gradient
    G entering the Linear, so dW = GᵀX moves by at most 2^-8·|G|ᵀ|X|, db by
    2^-8·Σ|G|, and dX = G·W by 2^-8·|G|·|W| plus its own bf16 rounding."""
    from distributed_compute_pytorch_amd.ops import apply_rope_qkv, rope_table
    from distributed_compute_pytorch_amd.ops.linear import FusedLinear, packed_linear
    from distributed_compute_pytorch_amd.ops.rope import rope_qkv_reference

    torch.manual_seed(0)
    heads, B, T = 2, 2, 64
    C = heads * 64
    table = rope_table(64, 10000.0, cuda)
    layers = [FusedLinear(C, C).to(cuda) for _ in range(3)]
    x0 = torch.randn(B, T, C, device=cuda).to(BF)
    wsum = torch.randn(B, T, 3 * C, device=cuda)

    def run(mode):
        for l in layers:
            l.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_()
        qkv = packed_linear(x, layers)
        assert qkv.dtype == BF
        if mode == "torch":
            y = rope_qkv_reference(qkv, heads, table)
        else:
            y = apply_rope_qkv(qkv, heads, table, inplace=(mode == "inplace"))
            assert (y.data_ptr() == qkv.data_ptr()) == (mode == "inplace")
        (y.float() * wsum).sum().backward()
        return (y.detach().clone(), x.grad.clone(), torch.cat([l.weight.grad for l in layers], 0).clone(),
                torch.cat([l.bias.grad for l in layers], 0).clone())

    yi, dxi, dwi, dbi = run("inplace")
    yo, dxo, dwo, dbo = run("outofplace")
    yt, dxt, dwt, dbt = run("torch")
    assert torch.equal(yi, yo)
    torch.testing.assert_close(dxi.float(), dxo.float(), rtol=2.0 ** -7, atol=1e-6)
    torch.testing.assert_close(dwi, dwo, rtol=1e-5, atol=1e-5 * float(dwo.abs().max()))
    torch.testing.assert_close(dbi, dbo, rtol=1e-5, atol=1e-5 * float(dbo.abs().max()))
    # against the PyTorch path, with the bound of the docstring
    G = _rope_ref64(wsum.to(BF), heads, table, inverse=True)
    G = torch.cat([G, wsum.to(BF)[..., 2 * C:].double()], -1).reshape(-1, 3 * C).abs()
    X = x0.double().reshape(-1, C).abs()
    W = torch.cat([l.weight.detach() for l in layers], 0).double().abs()
    u = 2.0 ** -8
    assert bool(((dwi.double() - dwt.double()).abs() <= u * (G.t() @ X) + 1e-6).all())
    assert bool(((dbi.double() - dbt.double()).abs() <= u * G.sum(0) + 1e-6).all())
    bound_x = (u * (G @ W)).reshape(B, T, C) + 2 * u * dxt.double().abs() + 1e-6
    assert bool(((dxi.double() - dxt.double()).abs() <= bound_x).all())


# ---------------------------------------------------------------- SwiGLU ---
def _swiglu_ref64(p, dy):
    F = p.shape[-1] // 2
    g, u, d = p[..., :F].double(), p[..., F:].double(), dy.double()
    sig = torch.sigmoid(g)
    return g * sig * u, torch.cat([d * u * sig * (1 + g * (1 - sig)), d * g * sig], -1)


@pytest.mark.parametrize("F", [8, 2048, 2056])
@pytest.mark.parametrize("M", [1, 77])
def test_swiglu_matches_fp64(cuda, M, F):
    from distributed_compute_pytorch_amd.ops import swiglu

    torch.manual_seed(0)
    p = (torch.randn(M, 2 * F, device=cuda) * 2).to(BF).requires_grad_()
    dy = torch.randn(M, F, device=cuda).to(BF)
    y = swiglu(p)
    assert y.shape == (M, F) and y.dtype == BF
    y.backward(dy)
    yr, dpr = _swiglu_ref64(p.detach(), dy)
    torch.testing.assert_close(y.double(), yr, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(p.grad[:, :F].double(), dpr[:, :F], rtol=1e-2, atol=2e-2)  # d_gate
    torch.testing.assert_close(p.grad[:, F:].double(), dpr[:, F:], rtol=1e-2, atol=2e-2)  # d_up


def test_swiglu_saturated_gates_stay_finite(cuda):
    from distributed_compute_pytorch_amd.ops import swiglu

    torch.manual_seed(0)
    F = 64
    gate = torch.linspace(-30, 30, 3 * F, device=cuda).reshape(3, F)
    gate = torch.cat([gate, torch.tensor([[-100.0, 100.0, -30.0, 30.0] * (F // 4)], device=cuda)], 0)
    up = torch.randn(4, F, device=cuda) * 3
    p = torch.cat([gate, up], -1).to(BF).requires_grad_()
    dy = torch.randn(4, F, device=cuda).to(BF)
    y = swiglu(p)
    y.backward(dy)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(p.grad).all())
    yr, dpr = _swiglu_ref64(p.detach(), dy)
    torch.testing.assert_close(y.double(), yr, rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(p.grad.double(), dpr, rtol=1e-2, atol=2e-2)


def test_swiglu_unsupported_shapes_fall_back(cuda):
    from distributed_compute_pytorch_amd.ops import swiglu

    torch.manual_seed(0)
    for p in ((torch.randn(5, 2 * 12, device=cuda) * 2).to(BF), torch.randn(5, 2 * 16, device=cuda) * 2):
        p = p.requires_grad_()
        dy = torch.randn(5, p.shape[1] // 2, device=cuda).to(p.dtype)
        y = swiglu(p)
        y.backward(dy)
        yr, dpr = _swiglu_ref64(p.detach(), dy)
        tol = dict(rtol=1e-2, atol=2e-2) if p.dtype == BF else dict(rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(y.double(), yr, **tol)
        torch.testing.assert_close(p.grad.double(), dpr, **tol)


# --------------------------------------------------------------- capture ---
@pytest.mark.parametrize("op", ["rms_norm", "rms_norm_dual", "rope", "rope_inplace", "swiglu"])
def test_captured_llama_op_replays_equal_eager(cuda, op):
    """Each op captured alone on one stream (forward + backward), replayed
    twice with changed inputs: every replay equals the eager call's bits."""
    from distributed_compute_pytorch_amd.ops import FusedRMSNorm, apply_rope_qkv, rope_table, swiglu

    torch.manual_seed(0)
    heads, T = 2, 64
    table = rope_table(64, 10000.0, cuda)
    norm = FusedRMSNorm(768).to(cuda)
    shape = {"rms_norm": (67, 768), "rms_norm_dual": (67, 768), "rope": (2, T, 3 * heads * 64),
             "rope_inplace": (2, T, 3 * heads * 64), "swiglu": (33, 2 * 256)}[op]
    gshape = (33, 256) if op == "swiglu" else shape
    x = torch.randn(shape, device=cuda).to(BF).requires_grad_()
    g = torch.randn(gshape, device=cuda).to(BF)

    def fn():
        x.grad = None
        norm.weight.grad = None
        if op == "rms_norm":
            y = norm(x)
            y.backward(g)
            return [y.detach(), x.grad, norm.weight.grad]
        if op == "rms_norm_dual":
            y, alias = norm.forward_dual(x)
            torch.autograd.backward([y, alias], [g, g])
            return [y.detach(), x.grad, norm.weight.grad]
        if op.startswith("rope"):
            y = apply_rope_qkv(x * 1, heads, table, inplace=(op == "rope_inplace"))
            y.backward(g)
            return [y.detach(), x.grad]
        y = swiglu(x)
        y.backward(g)
        return [y.detach(), x.grad]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s, capture_error_mode="thread_local"):
        out = fn()
    for i in range(2):
        with torch.no_grad():
            x.copy_(torch.randn(shape, device=cuda) * (i + 2))
            g.copy_(torch.randn(gshape, device=cuda))
        gr.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in out]
        ref = [t.clone() for t in fn()]
        for a, r in zip(got, ref):
            assert torch.equal(a, r)


# ----------------------------------------------------------------- model ---
def _tiny_cfg():
    from distributed_compute_pytorch_amd.models.llama import LlamaConfig

    return LlamaConfig(vocab=512, n_layer=2, n_head=2, n_embd=128, ffn_hidden=256, block_size=128)


def test_llama_fused_matches_plain_fp32(cuda):
    """fused=True under bf16 autocast against the fused=False model with fp32
    weights in fp32; the noise floor is the plain model's own bf16-autocast
    run against that reference (the bound of the GPT-2 comparisons:
    err < 4·noise + 2e-2)."""
    from distributed_compute_pytorch_amd.models.llama import LlamaForCausalLM

    torch.manual_seed(0)
    fused = LlamaForCausalLM(_tiny_cfg(), fused=True).to(cuda)
    plain = LlamaForCausalLM(_tiny_cfg(), fused=False).to(cuda)
    plain.load_state_dict(fused.state_dict())
    idx = torch.randint(0, 512, (2, 128), device=cuda)
    tgt = idx.roll(-1, 1)

    def run(m, amp):
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF, enabled=amp):
            loss = m(idx, tgt)
        loss.backward()
        return float(loss.detach()), {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}

    l_ref, g_ref = run(plain, False)
    l_noise, g_noise = run(plain, True)
    l_fused, g_fused = run(fused, True)
    print(f"loss ref {l_ref:.6f} plain-bf16 {l_noise:.6f} fused {l_fused:.6f}")
    assert abs(l_fused - l_ref) < 4 * abs(l_noise - l_ref) + 2e-2 * max(1.0, abs(l_ref)), (l_fused, l_noise, l_ref)
    assert set(g_fused) == set(g_ref)
    for n, r in g_ref.items():
        den = float(r.norm().clamp_min(1e-3))
        err = float((g_fused[n] - r).norm()) / den
        noise = float((g_noise[n] - r).norm()) / den
        print(f"{n}: fused err {err:.3e} plain-bf16 noise {noise:.3e}")
        assert err < 4 * noise + 2e-2, (n, err, noise)


def test_captured_llama_step_matches_eager(cuda):
    """Fused Llama (packed bias-free linears, RMSNorm, RoPE, flash attention,
    SwiGLU, head + loss, capturable AdamW): 4 replays of the captured step
    track 4 eager steps from the same start."""
    import distributed_compute_pytorch_amd as dcp
    from distributed_compute_pytorch_amd.models.llama import LlamaForCausalLM
    from distributed_compute_pytorch_amd.utils.graphs import CapturedStep, capture_stream

    torch.manual_seed(0)
    base = LlamaForCausalLM(_tiny_cfg(), fused=True).to(cuda)
    m_e, m_g = copy.deepcopy(base), copy.deepcopy(base)
    o_e = dcp.optim.AdamW(m_e.parameters(), lr=1e-3, weight_decay=0.1, capturable=True)
    s = capture_stream()
    with torch.cuda.stream(s):
        o_g = dcp.optim.AdamW(m_g.parameters(), lr=1e-3, weight_decay=0.1, capturable=True)
    gen = torch.Generator().manual_seed(1)
    batches = []
    for _ in range(6):
        t = torch.randint(0, 512, (4, 129), generator=gen)
        batches.append((t[:, :-1].contiguous().to(cuda), t[:, 1:].contiguous().to(cuda)))

    def make(m, opt):
        def run(x, y):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=BF):
                loss = m(x, y)
            loss.backward()
            opt.step()
            return loss
        return run

    run_e, run_g = make(m_e, o_e), make(m_g, o_g)
    for _ in range(2):
        run_e(*batches[0])
    cap = CapturedStep(run_g, [t.clone() for t in batches[0]], warmup=2, stream=s)
    for b in batches[1:5]:
        le = float(run_e(*b).detach())
        lg = float(cap(*b).detach())
        assert abs(le - lg) < 2e-2 * max(1.0, abs(le)), (le, lg)
    pe = torch.cat([p.detach().float().reshape(-1) for p in m_e.parameters()])
    pg = torch.cat([p.detach().float().reshape(-1) for p in m_g.parameters()])
    assert bool(torch.isfinite(pg).all())
    assert float((pe - pg).norm() / pe.norm()) < 1e-2
