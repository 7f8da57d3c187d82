"""The LAMB / LARS HIP kernels (mt_lamb_norms / mt_lamb_ratio / mt_lamb_update,
mt_lars_norms / mt_lars_update) vs the fp64 references of
tests/layerwise_ref.py, the CPU path of the same ops, bitwise repeatability,
the bf16 shadow and HIP-graph capture. Tensor list and tolerances: see
layerwise_ref (docstring and ``tolerances``)."""
import pytest
import torch

import layerwise_ref as lw

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
CASES = [("lamb", "default"), ("lamb", "maximize_scaled"), ("lamb", "clipped_scaled_adapt"),
         ("lars", "default"), ("lars", "nesterov_adapt"), ("lars", "dampening_maximize")]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,case", CASES)
def test_optimizer_matches_fp64(cuda, kind, case, dtype):
    lw.check_optimizer(kind, case, cuda, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,case", [("lamb", "always_adapt"), ("lamb", "no_bias_correction"),
                                       ("lamb", "clipped"), ("lars", "default"), ("lars", "no_momentum")])
def test_ratios_match_fp64(cuda, kind, case, dtype):
    ratios = lw.check_op_ratios(kind, case, cuda, dtype)
    r0 = ratios[0].cpu()
    assert float(r0[8]) == 1.0 and float(r0[lw.ZERO_GRAD]) == 1.0
    assert bool(torch.isfinite(torch.stack(ratios)).all())
    assert float(r0[7]) != 1.0  # (300, 8192): more chunks than the reduce workgroup has threads


def test_f16_parameters(cuda):
    """fp16 parameters go through the third Acc<> instantiation: one step from
    identical inputs against the fp64 formula, at fp16's spacing."""
    ps, _, ratios = lw.run_op("lamb", "default", cuda, torch.float16, steps=1)
    p = [x.double() for x in lw.make_params(cuda, torch.float16)]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    want = lw.lamb_ref_step(p, lw.make_grads(cuda, torch.float16, 0), m, v, 1, lw.lamb_cfg("default"))
    torch.testing.assert_close(ratios[0].double().cpu(), torch.tensor(want, dtype=torch.float64), rtol=1e-5, atol=0)
    for a, b in zip(ps, p):
        torch.testing.assert_close(a.double(), b, rtol=2e-3, atol=2e-3)  # 2 ulp of fp16 (2^-10 spacing)


@pytest.mark.parametrize("kind,case", [("lamb", "always_adapt"), ("lars", "nesterov_adapt")])
def test_bitwise_repeatable(cuda, kind, case):
    runs = []
    for _ in range(2):
        ps, (m, v), ratios = lw.run_op(kind, case, cuda, torch.float32, steps=2)
        runs.append(ps + m + v + ratios)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,case", [("lamb", "always_adapt"), ("lars", "nesterov_adapt")])
def test_gpu_matches_cpu_path(cuda, kind, case, dtype):
    gp, (gm, gv), gr = lw.run_op(kind, case, cuda, dtype, steps=2)
    cp, (cm, cv), cr = lw.run_op(kind, case, torch.device("cpu"), dtype, steps=2)
    tol = lw.tolerances(dtype)
    for a, b in zip(gp + gm + gv, cp + cm + cv):
        torch.testing.assert_close(a.cpu().float(), b.float(), **tol)
    torch.testing.assert_close(gr[0].cpu(), cr[0], rtol=1e-5, atol=0)
    torch.testing.assert_close(gr[1].cpu(), cr[1], rtol=1e-5 if dtype == torch.float32 else 3e-2, atol=0)


def test_lamb_rewrites_bf16_shadow(cuda):
    import distributed_compute_pytorch_amd as dcp
    from distributed_compute_pytorch_amd.optim.fused import fresh_bf16_shadow, register_bf16_shadow

    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(s, generator=g).to(cuda) for s in [(129, 65), (8193,), (5,)]]
    shadows = [torch.zeros_like(p, dtype=torch.bfloat16) for p in ps[:2]]
    for p, s in zip(ps, shadows):
        register_bf16_shadow(p, s)
    opt = dcp.optim.LAMB(ps, lr=1e-2)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(cuda)
    before = [p.clone() for p in ps]
    opt.step()
    for p, s, b in zip(ps, shadows, before):
        assert not torch.equal(p, b)
        assert torch.equal(s, p.to(torch.bfloat16))
        assert fresh_bf16_shadow(p) is s
    assert fresh_bf16_shadow(ps[2]) is None


def _capture_vs_eager(cuda, kind):
    """1 eager step + 3 replays of the captured step (fresh gradients copied
    into static buffers) vs 4 eager steps: the same kernels, so the same bits."""
    cfg = lw.lamb_cfg("always_adapt") if kind == "lamb" else lw.lars_cfg("nesterov_adapt")
    extra = {"capturable": True} if kind == "lamb" else {}
    dt = torch.float32
    pe, pg = lw.make_params(cuda, dt), lw.make_params(cuda, dt)
    oe, og = lw.make_optimizer(kind, pe, cfg, **extra), lw.make_optimizer(kind, pg, cfg, **extra)
    for it in range(lw.STEPS):
        lw.set_grads(pe, lw.make_grads(cuda, dt, it))
        oe.step()
    static = lw.make_grads(cuda, dt, 0)
    lw.set_grads(pg, static)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        og.step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    for st, g in zip(static, lw.make_grads(cuda, dt, 1)):
        st.copy_(g)
    torch.cuda.synchronize()
    with torch.cuda.graph(gr, stream=s, capture_error_mode="thread_local"):
        og.step()
    for it in range(1, lw.STEPS):
        for st, g in zip(static, lw.make_grads(cuda, dt, it)):
            st.copy_(g)
        gr.replay()
    torch.cuda.synchronize()
    for a, b in zip(pe, pg):
        assert torch.equal(a, b)
    return oe, og, pe, pg


def test_captured_lamb_equals_eager(cuda):
    oe, og, pe, pg = _capture_vs_eager(cuda, "lamb")
    for a, b in zip(pe, pg):
        se, sg = oe.state[a], og.state[b]
        assert sg["step"].is_cuda and float(sg["step"]) == lw.STEPS == float(se["step"])
        assert torch.equal(se["exp_avg"], sg["exp_avg"]) and torch.equal(se["exp_avg_sq"], sg["exp_avg_sq"])


def test_captured_lars_equals_eager(cuda):
    oe, og, pe, pg = _capture_vs_eager(cuda, "lars")
    for a, b in zip(pe, pg):
        assert torch.equal(oe.state[a]["momentum_buffer"], og.state[b]["momentum_buffer"])


def test_non_capturable_lamb_raises_in_capture(cuda):
    import distributed_compute_pytorch_amd as dcp

    p = torch.randn(100, device=cuda)
    p.grad = torch.randn(100, device=cuda)
    opt = dcp.optim.LAMB([p], lr=1e-3)
    opt.step()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="capturable=True"):
        with torch.cuda.graph(gr, stream=s, capture_error_mode="thread_local"):
            opt.step()
