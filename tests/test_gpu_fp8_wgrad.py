"""fp8 weight gradient on the GPU (csrc/kernels/gemm_fp8_wgrad.hip): the
transposing column quantiser and the split-K fp8 GEMM against
``quantize_cols_t_reference`` + fp64 matmuls, ``fp8_linear(wgrad="fp8")`` end to
end, graph replay, and a tiny ``LlamaConfig(fp8=True, fp8_wgrad=True)`` model."""
import functools

import pytest
import torch
from test_fp8_cpu import check_quantised, edge_rows
from test_gpu_fp8 import deq, linear_case, rel

from distributed_compute_pytorch_amd.ops.fp8 import (_FMT, fp8_linear, quantize_cols_t, quantize_cols_t_reference,
                                                     quantize_weight)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("C", [64, 192])
@pytest.mark.parametrize("M", [1, 33, 128, 200, 300])
def test_cols_quantiser_kernel(cuda, M, C, fmt):
    from distributed_compute_pytorch_amd._ext import C as _C

    x = edge_rows(M, C + 32, seed=M + C).to(cuda)[:, 16:16 + C]  # a row-strided view
    q, s = _C.fp8_quant_cols_t(x, _FMT[fmt][0])
    Mp = -(-M // 128) * 128
    assert q.shape == (C, Mp) and q.dtype == _FMT[fmt][1] and s.shape == (C,) and s.dtype == torch.float32
    check_quantised(x.t(), q[:, :M], s, fmt)
    assert not q.view(torch.uint8)[:, M:].any()
    q2, s2 = quantize_cols_t(x, fmt)  # the public entry point reaches the same kernel
    assert torch.equal(q2.view(torch.uint8), q.view(torch.uint8)) and torch.equal(s2, s)


@pytest.mark.parametrize("a_fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("M", [1, 200, 384, 1024])
@pytest.mark.parametrize("N,K", [(64, 64), (192, 64), (64, 192), (192, 192)])
def test_wgrad_gemm_kernel(cuda, N, K, M, a_fmt):
    """|c − ref| ≤ 2^-22·|ref| + Mp·2^-23·(|A| @ |B|ᵀ): exact fp8 products, fp32
    sums of at most Mp terms plus up to S slab adds, two scale multiplies and
    one add into the preload. Operands quantised on the CPU, so only the GEMM is
    under test; every split count, stored and accumulated, each run twice."""
    from distributed_compute_pytorch_amd._ext import C as _C

    g = torch.Generator().manual_seed(M + N + K)
    a8, sa = quantize_cols_t_reference(torch.randn(M, N, generator=g).to(torch.bfloat16), a_fmt)
    b8, sb = quantize_cols_t_reference(torch.randn(M, K, generator=g).to(torch.bfloat16), "e4m3")
    pre = torch.randn(N, K, generator=g)
    Mp = a8.shape[1]
    A, B = deq(a8, sa), deq(b8, sb)
    prod, slack = A @ B.t(), Mp * 2.0 ** -23 * (A.abs() @ B.abs().t())
    ops = (a8.to(cuda), sa.to(cuda), b8.to(cuda), sb.to(cuda), _FMT[a_fmt][0])
    for S in sorted({0, 1, 2, 3, Mp // 128}):
        if S > Mp // 128:
            continue
        for acc in (False, True):
            ref = prod + (pre.double() if acc else 0.0)
            run = lambda: _C.gemm_fp8_wgrad(*ops, accumulate_into=pre.to(cuda) if acc else None, splits=S)
            c = run()
            assert c.shape == (N, K) and c.dtype == torch.float32
            err, bound = (c.double().cpu() - ref).abs(), 2.0 ** -22 * ref.abs() + slack
            print(f"gemm_fp8_wgrad {N}x{K}x{M} {a_fmt} S={S} acc={acc}: worst fraction of the bound "
                  f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= bound).all())
            assert torch.equal(run(), c)


@functools.lru_cache(maxsize=None)
def wgrad_case(M, N, K, grad_fmt):
    """``linear_case`` plus the CPU emulation of the fp8 weight gradient: its
    dequantised operands and its relative L2 error against the fp64 dW."""
    inputs, refs, _ = linear_case(M, N, K, grad_fmt)
    x, gy = inputs[0], inputs[3]
    G, X = deq(*quantize_cols_t_reference(gy, grad_fmt)), deq(*quantize_cols_t_reference(x, "e4m3"))
    return inputs, refs, (G, X), rel(G @ X.t(), refs[2])


@pytest.mark.parametrize("grad_fmt", ["e5m2", "e4m3"])
@pytest.mark.parametrize("M,N,K", [(200, 192, 512), (33, 64, 256)])
def test_fp8_linear_wgrad_matches_fp64(cuda, M, N, K, grad_fmt):
    """dW within 1.5× the CPU emulation's own error against the fp64 dW (the
    margin of test_fp8_linear_matches_fp64: tie flips from one-ulp scale
    differences); y and dx bitwise those of wgrad="bf16"; db on the bf16 path;
    a second backward adds into the fp32 .grad in place."""
    (x, w, b, gy), (_, _, dw, db), (G, X), edw = wgrad_case(M, N, K, grad_fmt)
    outs = {}
    for wgrad in ("bf16", "fp8"):
        xa = x.to(cuda).requires_grad_(True)
        wa, ba = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
        y = fp8_linear(xa, wa, ba, grad_fmt=grad_fmt, wgrad=wgrad)
        y.backward(gy.to(cuda))
        outs[wgrad] = (y, xa, wa, ba)
    y, xa, wa, ba = outs["fp8"]
    assert torch.equal(y, outs["bf16"][0]) and torch.equal(xa.grad, outs["bf16"][1].grad)
    rdw = rel(wa.grad, dw)
    print(f"fp8_linear wgrad=fp8 {M}x{N}x{K} {grad_fmt}: dW {rdw:.4f} (emulation {edw:.4f}, ratio {rdw / edw:.3f})")
    assert wa.grad.dtype == torch.float32 and rdw <= 1.5 * edw
    assert not torch.equal(wa.grad, outs["bf16"][2].grad)
    assert ba.grad.dtype == torch.float32 and rel(ba.grad, db) < 1e-3
    g1 = wa.grad.clone()
    fp8_linear(xa, wa, ba, grad_fmt=grad_fmt, wgrad="fp8").backward(gy.to(cuda))
    Mp = -(-M // 128) * 128
    bound = 2.0 ** -22 * (2 * g1.double().cpu()).abs() + 2 * Mp * 2.0 ** -23 * (G.abs() @ X.abs().t())
    assert bool(((wa.grad.double().cpu() - 2 * g1.double().cpu()).abs() <= bound).all())


def test_fp8_linear_wgrad_graph_replay_equals_eager(cuda):
    (x, w, b, gy), _, _, _ = wgrad_case(200, 192, 512, "e5m2")
    w, b, gy = w.to(cuda).requires_grad_(True), b.to(cuda), gy.to(cuda)
    w8 = quantize_weight(w.detach().to(torch.bfloat16))
    xs = torch.zeros_like(x, device=cuda).requires_grad_(True)

    def run():
        y = fp8_linear(xs, w, b, w8=w8, wgrad="fp8")
        return (y,) + torch.autograd.grad(y, (xs, w), gy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for scale in (1.0, -0.5, 3.0):  # several replays on fresh inputs
        with torch.no_grad():
            xs.copy_(x.to(cuda) * scale)
        graph.replay()
        for got, want in zip(captured, run()):
            assert torch.equal(got, want)
        assert float(captured[2].abs().max()) > 0


def test_tiny_llama_fp8_wgrad(cuda):
    """fp8 weight gradients of wo / w2 against the same model with bf16 ones:
    the forward is untouched; the two gradients differ by at most 3× the CPU
    emulation's error at (200, 192, 512) e5m2 (model activations are not
    Gaussian, and the twin's bf16 gradient carries its own rounding)."""
    from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM

    cfg = dict(vocab=512, n_layer=2, n_head=2, n_embd=128, ffn_hidden=256, block_size=64)
    torch.manual_seed(0)
    ref = LlamaForCausalLM(LlamaConfig(fp8=True, **cfg)).to(cuda)
    m = LlamaForCausalLM(LlamaConfig(fp8=True, fp8_wgrad=True, **cfg)).to(cuda)
    m.load_state_dict(ref.state_dict())
    idx = torch.randint(0, 512, (4, 64), device=cuda)
    tgt = torch.randint(0, 512, (4, 64), device=cuda)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, loss_ref = m(idx, tgt), ref(idx, tgt)
    loss.backward()
    loss_ref.backward()
    loss, loss_ref = float(loss.detach()), float(loss_ref.detach())
    assert abs(loss - loss_ref) <= 1e-6 * abs(loss_ref)
    allowance = 3 * wgrad_case(200, 192, 512, "e5m2")[3]
    grads = dict(ref.named_parameters())
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        if n.endswith(("wo.weight", "w2.weight")):
            r = rel(p.grad, grads[n].grad)
            print(f"tiny llama {n}: fp8 vs bf16 weight gradient {r:.4f} (allowance {allowance:.4f}, "
                  f"ratio to the emulation {3 * r / allowance:.3f})")
            assert r <= allowance and not torch.equal(p.grad, grads[n].grad)
