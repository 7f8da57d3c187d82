"""fp8 Linear on the GPU: the row quantiser and the row-scaled fp8 MFMA GEMM
(csrc/kernels/gemm_fp8.hip) against ``quantize_rows_reference`` + fp64 matmuls,
``fp8_linear`` end to end, and a tiny ``LlamaConfig(fp8=True)`` model."""
import pytest
import torch
from test_fp8_cpu import check_quantised, edge_rows

from distributed_compute_pytorch_amd.ops.fp8 import (_FMT, fp8_linear, quantize_rows, quantize_rows_reference,
                                                     quantize_weight)

pytestmark = pytest.mark.gpu


def deq(q, s):
    return q.float().double().cpu() * s.double().cpu()[:, None]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("K", [16, 128, 384, 4096])
@pytest.mark.parametrize("R", [1, 33, 200])
def test_quantiser_kernel(cuda, R, K, fmt):
    from distributed_compute_pytorch_amd._ext import C

    x = edge_rows(R, K + 32, seed=R + K).to(cuda)[:, 16:16 + K]  # a row-strided view
    q, s = C.fp8_quant_rows(x, _FMT[fmt][0])
    assert q.shape == (R, K) and q.dtype == _FMT[fmt][1] and s.shape == (R,) and s.dtype == torch.float32
    check_quantised(x, q, s, fmt)
    q2, s2 = quantize_rows(x, fmt)  # the public entry point reaches the same kernel
    assert torch.equal(q2.view(torch.uint8), q.view(torch.uint8)) and torch.equal(s2, s)


@pytest.mark.parametrize("a_fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("K", [128, 192, 384, 1024])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("M", [1, 33, 128, 200])
def test_gemm_kernel(cuda, M, N, K, bias, a_fmt):
    """|c − ref| ≤ 2^-8·|ref| + K·2^-23·S, S = sa·sb·Σ|a||b|: exact fp8 products,
    fp32 sums of K terms, two scale multiplies and the bias add, one bf16
    rounding. Operands quantised on the CPU, so only the GEMM is under test."""
    from distributed_compute_pytorch_amd._ext import C

    g = torch.Generator().manual_seed(M + N + K)
    a8, sa = quantize_rows_reference(torch.randn(M, K, generator=g).to(torch.bfloat16), a_fmt)
    b8, sb = quantize_rows_reference((0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16), "e4m3")
    bv = torch.randn(N, generator=g) * 0.1 if bias else None
    A, B = deq(a8, sa), deq(b8, sb)
    ref = A @ B.t() + (bv.double() if bias else 0.0)
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (A.abs() @ B.abs().t())
    args = (a8.to(cuda), sa.to(cuda), b8.to(cuda), sb.to(cuda), bv.to(cuda) if bias else None, _FMT[a_fmt][0])
    c = C.gemm_fp8(*args)
    assert c.shape == (M, N) and c.dtype == torch.bfloat16
    err = (c.double().cpu() - ref).abs()
    print(f"gemm_fp8 {M}x{N}x{K} bias={bias} {a_fmt}: worst fraction of the bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(C.gemm_fp8(*args), c)


def linear_case(M, N, K, grad_fmt):
    """Inputs, the fp64 Linear on them and the CPU emulation's relative L2 errors."""
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = 0.02 * torch.randn(N, K, generator=g)
    b = 0.1 * torch.randn(N, generator=g)
    gy = torch.randn(M, N, generator=g).to(torch.bfloat16)
    w16 = w.to(torch.bfloat16)
    y = x.double() @ w16.double().t() + b.double()
    dx = gy.double() @ w16.double()
    dw, db = gy.double().t() @ x.double(), gy.double().sum(0)
    y_emu = deq(*quantize_rows_reference(x)) @ deq(*quantize_rows_reference(w16)).t() + b.double()
    dx_emu = deq(*quantize_rows_reference(gy, grad_fmt)) @ deq(*quantize_rows_reference(w16.t().contiguous())).t()
    return (x, w, b, gy), (y, dx, dw, db), (rel(y_emu, y), rel(dx_emu, dx))


@pytest.mark.parametrize("grad_fmt", ["e5m2", "e4m3"])
@pytest.mark.parametrize("M,N,K", [(200, 192, 512), (33, 64, 256)])
def test_fp8_linear_matches_fp64(cuda, M, N, K, grad_fmt):
    """y and dx within 1.5× the CPU emulation's own error against the fp64
    Linear (the margin: tie flips from one-ulp scale differences and the bf16
    output rounding); dw / db on the unchanged bf16 path, at its tolerances."""
    (x, w, b, gy), (y, dx, dw, db), (ey, edx) = linear_case(M, N, K, grad_fmt)
    xa = x.to(cuda).requires_grad_(True)
    wa, ba = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    out = fp8_linear(xa, wa, ba, grad_fmt=grad_fmt)
    out.backward(gy.to(cuda))
    ry, rdx = rel(out, y), rel(xa.grad, dx)
    print(f"fp8_linear {M}x{N}x{K} {grad_fmt}: y {ry:.4f} (emulation {ey:.4f}), dx {rdx:.4f} (emulation {edx:.4f})")
    assert out.dtype == torch.bfloat16 and ry <= 1.5 * ey
    assert rdx <= 1.5 * edx
    assert wa.grad.dtype == torch.float32 and rel(wa.grad, dw) < 1e-2
    assert ba.grad.dtype == torch.float32 and rel(ba.grad, db) < 1e-3


def test_fp8_linear_graph_replay_equals_eager(cuda):
    (x, w, b, gy), _, _ = linear_case(200, 192, 512, "e5m2")
    w, b, gy = w.to(cuda), b.to(cuda), gy.to(cuda)
    w8 = quantize_weight(w.to(torch.bfloat16))
    xs = torch.zeros_like(x, device=cuda).requires_grad_(True)

    def run():
        y = fp8_linear(xs, w, b, w8=w8)
        return y, torch.autograd.grad(y, xs, gy)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yg, dxg = run()
    for scale in (1.0, -0.5, 3.0):  # several replays on fresh inputs
        with torch.no_grad():
            xs.copy_(x.to(cuda) * scale)
        graph.replay()
        ye, dxe = run()
        assert torch.equal(yg, ye) and torch.equal(dxg, dxe)
        assert float(ye.float().abs().max()) > 0


# |loss(fp8) − loss(bf16)| of the tiny model below, measured on an MI355X at the
# two seeds: 0: 8.87e-5, 1: 3.75e-4 (losses 6.28 and 6.26; NOTES §45). A CPU
# emulation of wo / w2 is not a usable allowance here: both GPU models round
# through bf16 at every op, and a perturbed branch flips those roundings, which
# an fp32 emulation does not see. The bound is 3× the larger measured
# difference, at both seeds.
LLAMA_LOSS_ALLOWANCE = 3 * 3.75e-4


@pytest.mark.parametrize("seed", [0, 1])
def test_tiny_llama_fp8(cuda, seed):
    from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM

    cfg = dict(vocab=512, n_layer=2, n_head=2, n_embd=128, ffn_hidden=256, block_size=64)
    torch.manual_seed(seed)
    ref = LlamaForCausalLM(LlamaConfig(**cfg)).to(cuda)
    m = LlamaForCausalLM(LlamaConfig(fp8=True, **cfg)).to(cuda)
    m.load_state_dict(ref.state_dict())
    idx = torch.randint(0, 512, (4, 64), device=cuda)
    tgt = torch.randint(0, 512, (4, 64), device=cuda)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, loss_ref = m(idx, tgt), ref(idx, tgt)
    loss.backward()
    print(f"tiny llama seed {seed}: loss {float(loss):.6f}, bf16 model {float(loss_ref):.6f}, "
          f"difference {abs(float(loss) - float(loss_ref)):.2e}")
    assert torch.isfinite(loss)
    assert abs(float(loss) - float(loss_ref)) <= LLAMA_LOSS_ALLOWANCE
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
