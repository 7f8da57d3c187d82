"""conv3's backward with BN3's backward apply as the kernel's prologue
(csrc/kernels/conv3_bwd.hip, `_C.conv3_bwd_fused`) against today's unfused
composition `bn_bwd_apply_g` -> `conv1x1_dgrad_bnred` (+ `conv1x1_wgrad`).

Oracle: fp64 torch on the same bf16 inputs — dz3 from the BN-backward formula
rounded to bf16, then dy2 = dz3·W3, the RED sums of the bf16-rounded dy2,
dW3 = dz3ᵀ·y2, dγ3 and dβ3. Error metric: relative L2 norm ‖a − o‖ / ‖o‖ per
output (a max-norm over a few thousand bf16 roundings is decided by single
elements; the L2 form compares the two paths' rounding and accumulation
noise as a whole). The fused path must stay within 1.5x the unfused path's
error measured in the same test; dz3, dγ3, dβ3 must match bit for bit.

Tiles are 32 rows: 25 rows = less than one tile, 50 = one tile + a ragged
tail, 162 = five tiles + a 2-row tail; `c3bwd_grid` = 2 makes each workgroup
run three tiles, so the register prefetch crosses tile boundaries.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN = 1.5


def _rel(a, o):
    return float((a.double() - o).norm() / o.norm().clamp_min(1e-30))


@pytest.fixture()
def tune():
    from distributed_compute_pytorch_amd import _C

    keys = ("c3bwd64", "c3bwd128", "c3bwd_grid")
    old = {k: _C.gemm_tune_get(k) for k in keys}

    def set_(**kv):
        for k, v in kv.items():
            _C.gemm_tune(k, v)

    yield set_
    for k, v in old.items():
        _C.gemm_tune(k, v)


def _case(dev, w, N, hw, dense):
    """bf16 operands of one conv3 backward. dense: g has no masked rows
    (gy2 = None upstream gives such a g only through the ReLU bits; here every
    element is kept), else about half of g is zero as after a ReLU mask."""
    C = 4 * w
    gen = torch.Generator(device="cpu").manual_seed(1000 * w + 10 * N * hw + int(dense))
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    cl = lambda t: t.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)  # noqa: E731
    z3 = cl(r(N, C, hw, hw) * 1.5 + 0.3)
    g = r(N, C, hw, hw) * 0.1
    if not dense:
        g = g * (torch.rand(N, C, hw, hw, generator=gen) > 0.5)
    g = cl(g)
    x2 = cl(r(N, w, hw, hw))
    wt = (r(w, C) * (C ** -0.5)).to(dev).to(torch.bfloat16).contiguous()  # W3ᵀ [w][4w]
    f = lambda t: t.to(dev).float().contiguous()  # noqa: E731
    gamma3, gamma2, beta2 = f(r(C) * 0.3 + 1), f(r(w) * 0.3 + 1), f(r(w) * 0.2)
    M = N * hw * hw
    zf = z3.permute(0, 2, 3, 1).reshape(M, C).double()
    gf = g.permute(0, 2, 3, 1).reshape(M, C).double()
    xf = x2.permute(0, 2, 3, 1).reshape(M, w).double()
    mean3, mean2 = zf.mean(0).float(), xf.mean(0).float()
    invstd3 = (zf.var(0, unbiased=False) + 1e-5).rsqrt().float()
    invstd2 = (xf.var(0, unbiased=False) + 1e-5).rsqrt().float()
    acc3 = torch.cat([gf.sum(0), (gf * (zf - mean3.double())).sum(0)]).float().contiguous()
    # the forward's y2 = relu(bn2(x2)) (bf16), conv3's A operand for dW3
    sc2 = gamma2 * invstd2
    sf2 = beta2 - mean2 * sc2
    y2 = torch.relu(x2.float() * sc2.view(1, w, 1, 1) + sf2.view(1, w, 1, 1)).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    # ---- fp64 oracle
    inv3 = invstd3.double()
    k1 = gamma3.double() * inv3
    k2 = acc3[:C].double() / M
    k3 = acc3[C:].double() / M * inv3 * inv3
    dz3_o = (k1 * (gf - k2 - (zf - mean3.double()) * k3)).to(torch.bfloat16).double()
    dy_o = dz3_o @ wt.double().t()  # [M, 4w] · [4w, w]
    mask = (x2.float().permute(0, 2, 3, 1).reshape(M, w) * sc2 + sf2) > 0
    g2 = dy_o.to(torch.bfloat16).double() * mask
    acc2_o = torch.cat([g2.sum(0), (g2 * (xf - mean2.double())).sum(0)])
    dw_o = dz3_o.t() @ y2.permute(0, 2, 3, 1).reshape(M, w).double()  # [C, w]
    ora = dict(dz3=dz3_o, dy=dy_o, acc2=acc2_o, dw=dw_o, dgamma=acc3[C:].double() * inv3, dbeta=acc3[:C].double())
    ops = dict(g=g, z3=z3, gamma3=gamma3, mean3=mean3.contiguous(), invstd3=invstd3.contiguous(), acc3=acc3, wt=wt,
               x2=x2, gamma2=gamma2, beta2=beta2, mean2=mean2.contiguous(), invstd2=invstd2.contiguous(), y2=y2)
    return ops, ora, M


_CASES = {}


def _cached_case(dev, *key):
    if key not in _CASES:
        _CASES[key] = _case(dev, *key)
    return _CASES[key]


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("grid", [0, 2])
@pytest.mark.parametrize("N,hw,dense", [(1, 5, False), (2, 5, False), (2, 9, False), (2, 9, True)])
@pytest.mark.parametrize("w", [64, 128])
def test_fused_matches_unfused_within_margin(cuda, tune, w, N, hw, dense, grid):
    from distributed_compute_pytorch_amd import _C

    if grid and N * hw * hw <= 64:
        grid = 1  # small cases: one workgroup runs every tile
    o, ora, M = _cached_case(cuda, w, N, hw, dense)
    tune(c3bwd64=1, c3bwd128=1, c3bwd_grid=grid)
    assert _C.conv3_bwd_mode(M, w) == 1
    # today's composition
    dz3_u, dg_u, db_u = _C.bn_bwd_apply_g(o["g"], o["z3"], o["gamma3"], o["mean3"], o["invstd3"], o["acc3"])
    dy_u, acc2_u = _C.conv1x1_dgrad_bnred(dz3_u, o["wt"], o["x2"], o["gamma2"], o["beta2"], o["mean2"], o["invstd2"])
    dw_u = _C.conv1x1_wgrad(dz3_u, o["y2"])
    # fused
    dy_f, acc2_f, dz3_f = _C.conv3_bwd_fused(o["g"], o["z3"], o["gamma3"], o["mean3"], o["invstd3"], o["acc3"],
                                             o["wt"], o["x2"], o["gamma2"], o["beta2"], o["mean2"], o["invstd2"])
    dw_f = _C.conv1x1_wgrad(dz3_f, o["y2"])
    dg_f, db_f = _C.bn_dparams(o["acc3"], o["invstd3"])
    torch.cuda.synchronize()
    assert torch.equal(dz3_f, dz3_u), "stored dz3 differs from bn_bwd_apply_g's"
    assert torch.equal(dg_f, dg_u) and torch.equal(db_f, db_u), "dgamma3 / dbeta3 differ"
    assert dy_f.shape == dy_u.shape and dy_f.is_contiguous(memory_format=torch.channels_last)
    errs = {
        "dz3": (_rel(_rows(dz3_f), ora["dz3"]), _rel(_rows(dz3_u), ora["dz3"])),
        "dy2": (_rel(_rows(dy_f), ora["dy"]), _rel(_rows(dy_u), ora["dy"])),
        "acc2": (_rel(acc2_f, ora["acc2"]), _rel(acc2_u, ora["acc2"])),
        "dW3": (_rel(dw_f.reshape(4 * w, w), ora["dw"]), _rel(dw_u.reshape(4 * w, w), ora["dw"])),
        "dgamma3": (_rel(dg_f, ora["dgamma"]), _rel(dg_u, ora["dgamma"])),
        "dbeta3": (_rel(db_f, ora["dbeta"]), _rel(db_u, ora["dbeta"])),
    }
    print(f"w={w} M={M} dense={dense} grid={grid} (fused, unfused) rel-L2 errors: "
          + ", ".join(f"{k}=({a:.3e}, {b:.3e})" for k, (a, b) in errs.items()))
    for k, (ef, eu) in errs.items():
        assert ef <= MARGIN * eu, (k, ef, eu)
    # the unfused error itself is bf16 rounding of the outputs, not garbage
    assert errs["dy2"][1] < 1e-2 and errs["dz3"][1] < 1e-2


def _stage(dev, w, seed=0):
    from distributed_compute_pytorch_amd.models import resnet as R

    torch.manual_seed(seed)
    st = R.BottleneckStage(R.Bottleneck(4 * w, w, fused_bn=True), R.Bottleneck(4 * w, w, fused_bn=True))
    for m in st.modules():
        if hasattr(m, "running_mean") and getattr(m, "weight", None) is not None:
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, 0.0, 0.2)
    return st.to(dev).to(memory_format=torch.channels_last).train()


def _run_chain(st, x, wgt):
    """The stage's blocks as ResNet._chain runs them (block 0's BN3 fused into
    block 1's conv1 node); returns the parameter gradients."""
    blocks = list(st)
    for p in st.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h, a, head = x, None, None
        for i, blk in enumerate(blocks):
            h, a, head = blk.chain(h, a, head, blocks[i + 1] if i + 1 < len(blocks) else None)
        loss = (h.float() * wgt).sum()
    loss.backward()
    return [p.grad for p in st.parameters()]


@pytest.mark.parametrize("w", [64, 128])
def test_stage_param_grads_on_vs_off(cuda, tune, w):
    """Two identity bottlenecks at 8x8: parameter gradients with the fused
    conv3 backward on and off against an fp64 run of the plain composition;
    on must stay within 1.5x off's error (relative L2 over all parameters)."""
    from distributed_compute_pytorch_amd import _C
    from distributed_compute_pytorch_amd.models import resnet as R
    from distributed_compute_pytorch_amd.ops import conv as OC

    st = _stage(cuda, w)
    gen = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(4, 4 * w, 8, 8, generator=gen).to(cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    wgt = torch.randn(4, 4 * w, 8, 8, generator=gen).to(cuda)
    ref = R.BottleneckStage(R.Bottleneck(4 * w, w, fused_bn=False), R.Bottleneck(4 * w, w, fused_bn=False)).to(cuda)
    ref.load_state_dict(st.state_dict())
    ref = ref.double().train()
    (ref(x.double()) * wgt.double()).sum().backward()
    gref = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])

    calls = {"n": 0}
    real = _C.conv3_bwd_fused

    def counted(*a):
        calls["n"] += 1
        return real(*a)

    res = {}
    for mode in (1, 0):
        tune(c3bwd64=mode, c3bwd128=mode)
        m = copy.deepcopy(st)
        calls["n"] = 0
        OC._C.conv3_bwd_fused, keep = counted, OC._C.conv3_bwd_fused
        try:
            grads = _run_chain(m, x, wgt)
        finally:
            OC._C.conv3_bwd_fused = keep
        assert calls["n"] == (1 if mode else 0), "the fused conv3 backward did not run exactly where it should"
        assert not OC._C3_DEFERRED, "deferred-gradient registry not empty after backward"
        res[mode] = torch.cat([g.double().reshape(-1) for g in grads])
    e_on, e_off = _rel(res[1], gref), _rel(res[0], gref)
    print(f"w={w}: parameter-gradient rel-L2 error vs fp64: fused {e_on:.3e}, unfused {e_off:.3e}")
    assert bool(torch.isfinite(res[1]).all())
    assert e_off < 0.5, e_off  # the fp64 composition is the same function (bf16 chain vs fp64: ~0.13 at 256 rows)
    assert e_on <= MARGIN * e_off, (e_on, e_off)


def test_stale_or_summed_gradient_raises(cuda, tune):
    """z3 with a second consumer: autograd sums the gradients, the conv3 node
    does not get the boundary's deferred gradient and must refuse it."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    tune(c3bwd64=1)
    st = _stage(cuda, 64)
    b0, b1 = list(st)
    x = torch.randn(2, 256, 8, 8, device=cuda).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        z1, s1 = OC.conv1x1(x, b0.conv1.weight, stats=True)
        x2, s2 = OC.bn_relu_conv(z1, b0.bn1, b0.conv2.weight, 3, 1, 1, sums=s1, stats=True)
        z3, s3 = OC.bn_relu_conv1x1(x2, b0.bn2, b0.conv3.weight, stats=True, sums=s2)
        y, z1n, _ = OC.bn_res_act_conv1x1(b0.bn3, z3, s3, x, b1.conv1.weight)
        loss = z1n.float().sum() + z3.float().sum()
    with pytest.raises(RuntimeError, match="conv3 backward fusion"):
        loss.backward()
    assert not OC._C3_DEFERRED


def test_fused_backward_replays_in_hip_graph(cuda, tune):
    """Forward + backward of the two-block chain captured once and replayed on
    new inputs: gradients equal an eager run on the same inputs, and the
    registry holds nothing after capture or replay."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    tune(c3bwd64=1)
    st = _stage(cuda, 64, seed=3)
    eager = copy.deepcopy(st)
    gen = torch.Generator(device="cpu").manual_seed(11)
    mk = lambda: torch.randn(4, 256, 8, 8, generator=gen).to(cuda).to(torch.bfloat16).contiguous(  # noqa: E731
        memory_format=torch.channels_last)
    wgt = torch.randn(4, 256, 8, 8, generator=gen).to(cuda)
    xs = mk()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run_chain(st, xs, wgt)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grads = _run_chain(st, xs, wgt)
    assert not OC._C3_DEFERRED, "registry holds tensors after capture"
    for _ in range(2):
        xn = mk()
        xs.copy_(xn)
        graph.replay()
        torch.cuda.synchronize()
        assert not OC._C3_DEFERRED
        # BN running statistics do not enter training-mode gradients: a fresh copy is an equal model
        want = _run_chain(copy.deepcopy(eager), xn, wgt)
        got = torch.cat([g.double().reshape(-1) for g in grads])
        exp = torch.cat([g.double().reshape(-1) for g in want])
        assert bool(torch.isfinite(got).all())
        # atomics order is the only difference between a replay and an eager run
        assert _rel(got, exp) < 1e-2, _rel(got, exp)
