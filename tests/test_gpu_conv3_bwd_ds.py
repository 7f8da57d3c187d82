"""conv3's backward at a downsample block, relu(bn3(z3) + bn_d(zd)), with both
BNs' backward applies as the kernel's prologue (csrc/kernels/conv3_bwd.hip
kDual / kDzd, `_C.conv3_bwd_ds_fused`) against the unfused composition
`bn_bwd_apply2_g` -> `conv1x1_dgrad_bnred` / `conv1x1_dgrad`.

Everything the kernel stores (dz3, dzd, dy2, and at w = 64 the downsample
conv's data gradient dx_d) and all four BN parameter gradients must match the
unfused path bit for bit. The RED sums (Σg2, Σg2·(x2 − μ2)) are fp32 atomics in
both paths; they are compared against an fp64 oracle over the same bf16 dy2 by
relative L2 error, the fused error at most 1.5x the unfused one (the bound of
test_gpu_conv3_bwd_fused.py for atomic-order differences).

Tiles are 32 rows: 25 rows = less than one tile, 50 = one tile + a ragged
tail, 162 = five tiles + a 2-row tail; `c3bwd_grid` = 1 / 2 makes a workgroup
walk several tiles, so the register prefetch crosses tile boundaries.
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

    keys = ("c3bwd64", "c3bwd128", "c3bwd_ds64", "c3bwd_ds128", "c3bwd_grid")
    old = {k: _C.gemm_tune_get(k) for k in keys}

    def set_(**kv):
        for k, v in kv.items():
            _C.gemm_tune(k, v)

    yield set_
    for k, v in old.items():
        _C.gemm_tune(k, v)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _case(dev, w, N, hw):
    """bf16 operands of one downsample-block conv3 backward; about half of g
    is zero, as after a ReLU mask."""
    C = 4 * w
    gen = torch.Generator(device="cpu").manual_seed(77 * w + 10 * N * hw)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    cl = lambda t: t.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)  # noqa: E731
    f = lambda t: t.to(dev).float().contiguous()  # noqa: E731
    z3, zd = cl(r(N, C, hw, hw) * 1.5 + 0.3), cl(r(N, C, hw, hw) * 0.7 - 0.2)
    g = cl(r(N, C, hw, hw) * 0.1 * (torch.rand(N, C, hw, hw, generator=gen) > 0.5))
    x2 = cl(r(N, w, hw, hw))
    wt = (r(w, C) * (C ** -0.5)).to(dev).to(torch.bfloat16).contiguous()   # W3ᵀ [w][4w]
    wdt = (r(w, C) * (C ** -0.5)).to(dev).to(torch.bfloat16).contiguous()  # Wdᵀ [w][4w]
    gamma3, gammad, gamma2, beta2 = f(r(C) * 0.3 + 1), f(r(C) * 0.3 + 1), f(r(w) * 0.3 + 1), f(r(w) * 0.2)
    M = N * hw * hw
    gf = _rows(g).double()

    def stats(t):
        tf = _rows(t).double()
        mean = tf.mean(0).float()
        invstd = (tf.var(0, unbiased=False) + 1e-5).rsqrt().float()
        acc = torch.cat([gf.sum(0), (gf * (tf - mean.double())).sum(0)]).float().contiguous()
        return mean.contiguous(), invstd.contiguous(), acc

    mean3, invstd3, acc3 = stats(z3)
    meand, invstdd, accd = stats(zd)
    xf = _rows(x2).double()
    mean2 = xf.mean(0).float().contiguous()
    invstd2 = (xf.var(0, unbiased=False) + 1e-5).rsqrt().float().contiguous()
    return dict(g=g, z3=z3, zd=zd, x2=x2, wt=wt, wdt=wdt, gamma3=gamma3, mean3=mean3, invstd3=invstd3, acc3=acc3,
                gammad=gammad, meand=meand, invstdd=invstdd, accd=accd, gamma2=gamma2, beta2=beta2, mean2=mean2,
                invstd2=invstd2, M=M)


_CASES = {}


def _unfused(dev, w, N, hw):
    """Operands, the unfused path's results and the fp64 RED oracle, computed
    once per shape and left unchanged."""
    from distributed_compute_pytorch_amd import _C

    key = (w, N, hw)
    if key not in _CASES:
        o = _case(dev, w, N, hw)
        dz3, dg3, db3, dzd, dgd, dbd = _C.bn_bwd_apply2_g(o["g"], o["z3"], o["gamma3"], o["mean3"], o["invstd3"],
                                                          o["acc3"], o["zd"], o["gammad"], o["meand"], o["invstdd"],
                                                          o["accd"])
        dy, acc2 = _C.conv1x1_dgrad_bnred(dz3, o["wt"], o["x2"], o["gamma2"], o["beta2"], o["mean2"], o["invstd2"])
        dxd = _C.conv1x1_dgrad(dzd, o["wdt"]) if w == 64 else None
        torch.cuda.synchronize()
        # fp64 RED sums of the bf16 dy2 the kernels stored, mask from the fp32 BN2 + ReLU forward
        sc2 = o["gamma2"] * o["invstd2"]
        sf2 = o["beta2"] - o["mean2"] * sc2
        xr = _rows(o["x2"])
        g2 = _rows(dy).double() * (torch.addcmul(sf2, xr.float(), sc2) > 0)
        acc2_o = torch.cat([g2.sum(0), (g2 * (xr.double() - o["mean2"].double())).sum(0)])
        _CASES[key] = (o, dict(dz3=dz3, dzd=dzd, dy=dy, dxd=dxd, acc2=acc2, dg3=dg3, db3=db3, dgd=dgd, dbd=dbd), acc2_o)
    return _CASES[key]


@pytest.mark.parametrize("grid", [0, 1, 2])
@pytest.mark.parametrize("N,hw", [(1, 5), (2, 5), (2, 9)])
@pytest.mark.parametrize("w", [64, 128])
def test_fused_matches_unfused(cuda, tune, w, N, hw, grid):
    from distributed_compute_pytorch_amd import _C

    tune(c3bwd64=1, c3bwd128=1, c3bwd_ds64=1, c3bwd_ds128=1, c3bwd_grid=0)
    o, u, acc2_o = _unfused(cuda, w, N, hw)
    tune(c3bwd_grid=grid)
    assert _C.conv3_bwd_ds_mode(o["M"], w) == (2 if w == 64 else 1)
    out = _C.conv3_bwd_ds_fused(o["g"], o["z3"], o["gamma3"], o["mean3"], o["invstd3"], o["acc3"], o["zd"],
                                o["gammad"], o["meand"], o["invstdd"], o["accd"], o["wt"],
                                o["wdt"] if w == 64 else None, o["x2"], o["gamma2"], o["beta2"], o["mean2"],
                                o["invstd2"])
    dg3, db3 = _C.bn_dparams(o["acc3"], o["invstd3"])
    dgd, dbd = _C.bn_dparams(o["accd"], o["invstdd"])
    torch.cuda.synchronize()
    assert len(out) == (5 if w == 64 else 4)
    dy, acc2, dz3, dzd = out[:4]
    assert torch.equal(dz3, u["dz3"]), "stored dz3 differs from bn_bwd_apply2_g's"
    assert torch.equal(dzd, u["dzd"]), "stored dzd differs from bn_bwd_apply2_g's"
    assert dy.shape == u["dy"].shape and dy.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(dy, u["dy"]), "dy2 differs from conv1x1_dgrad_bnred's"
    if w == 64:
        assert out[4].shape == u["dxd"].shape and out[4].is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(out[4], u["dxd"]), "dx_d differs from conv1x1_dgrad's"
    for a, b, name in ((dg3, u["dg3"], "dgamma3"), (db3, u["db3"], "dbeta3"), (dgd, u["dgd"], "dgamma_d"),
                       (dbd, u["dbd"], "dbeta_d")):
        assert torch.equal(a, b), name
    ef, eu = _rel(acc2, acc2_o), _rel(u["acc2"], acc2_o)
    print(f"w={w} M={o['M']} grid={grid}: RED sums rel-L2 error vs fp64: fused {ef:.3e}, unfused {eu:.3e}")
    assert eu < 1e-4, eu  # fp32 sums of at most 162 bf16 terms
    assert ef <= MARGIN * eu, (ef, eu)


# ---------------------------------------------------------------- stage level


def _stage(dev, w, stride=1, seed=0):
    """A downsample bottleneck (w → 4w channels at stride 1, 2w → 4w at stride 2)
    followed by an identity bottleneck."""
    from distributed_compute_pytorch_amd.models import resnet as R

    torch.manual_seed(seed)
    cin = w if stride == 1 else 2 * w
    st = R.BottleneckStage(R.Bottleneck(cin, w, stride, R._downsample(cin, 4 * w, stride, True), fused_bn=True),
                           R.Bottleneck(4 * w, w, fused_bn=True))
    for m in st.modules():
        if hasattr(m, "running_mean") and getattr(m, "weight", None) is not None:
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, 0.0, 0.2)
    return st.to(dev).to(memory_format=torch.channels_last).train()


def _ref_grads(st, x, wgt, w, stride):
    """fp64 run of the plain composition: input gradient + parameter gradients, flat."""
    from distributed_compute_pytorch_amd.models import resnet as R

    cin = x.shape[1]
    ref = R.BottleneckStage(R.Bottleneck(cin, w, stride, R._downsample(cin, 4 * w, stride, False), fused_bn=False),
                            R.Bottleneck(4 * w, w, fused_bn=False)).to(x.device)
    ref.load_state_dict(st.state_dict())
    ref = ref.double().train()
    xr = x.double().requires_grad_(True)
    (ref(xr) * wgt.double()).sum().backward()
    return torch.cat([xr.grad.reshape(-1)] + [p.grad.reshape(-1) for p in ref.parameters()])


def _inputs(dev, cin, cout, hw_out, seed=7):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    hw = 8
    x = torch.randn(4, cin, hw, hw, generator=gen).to(dev).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    return x, torch.randn(4, cout, hw_out, hw_out, generator=gen).to(dev)


def _flat(x, st):
    return torch.cat([x.grad.double().reshape(-1)] + [p.grad.double().reshape(-1) for p in st.parameters()])


def _run_chain(st, x, wgt):
    """The stage's blocks as ResNet._chain runs them (block 0's BN3 and
    downsample BN fused into block 1's conv1 node); input + parameter gradients."""
    blocks = list(st)
    for p in st.parameters():
        p.grad = None
    x = x.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h, a, head = x, None, None
        for i, blk in enumerate(blocks):
            h, a, head = blk.chain(h, a, head, blocks[i + 1] if i + 1 < len(blocks) else None)
        loss = (h.float() * wgt).sum()
    loss.backward()
    return _flat(x, st)


def _run_manual(st, x, wgt, ds_first, extra_consumer=False):
    """The same graph built by hand at w = 64 with the downsample conv node
    created before (ds_first) or after the main branch: autograd runs the
    later-created of two ready nodes first, so each order of the conv3 node and
    the downsample conv node occurs."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    b0, b1 = list(st)
    conv_d, bn_d = b0.downsample[0], b0.downsample[1]
    for p in st.parameters():
        p.grad = None
    x = x.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        if ds_first:
            zd, sd = OC.conv1x1(x, conv_d.weight, stats=True)
        z1, s1 = OC.conv1x1(x, b0.conv1.weight, stats=True)
        x2, s2 = OC.bn_relu_conv(z1, b0.bn1, b0.conv2.weight, 3, 1, 1, sums=s1, stats=True)
        z3, s3 = OC.bn_relu_conv1x1(x2, b0.bn2, b0.conv3.weight, stats=True, sums=s2)
        if not ds_first:
            zd, sd = OC.conv1x1(x, conv_d.weight, stats=True)
        y, z1n, s1n = OC.bn_res_act_conv1x1(b0.bn3, z3, s3, None, b1.conv1.weight, (bn_d, zd, sd))
        h, _, _ = b1.chain(y, None, (z1n, s1n), None)
        loss = (h.float() * wgt).sum()
        if extra_consumer:
            loss = loss + z3.float().sum()
    loss.backward()
    return _flat(x, st)


class _Spy:
    """Counts calls of `_C` entry points as ops/conv.py sees them and records
    the order in which the two marked nodes take a deferred entry."""

    def __init__(self, *names):
        from distributed_compute_pytorch_amd.ops import conv as OC

        self.OC, self.names, self.n, self.roles = OC, names, {k: 0 for k in names}, []

    def __enter__(self):
        OC = self.OC
        self.keep = {k: getattr(OC._C, k) for k in self.names}
        self.keep_take = OC._c3ds_take
        for k in self.names:
            setattr(OC._C, k, self._wrap(k, self.keep[k]))

        def take(ctx, gz, role):
            if getattr(ctx, "_c3ds", False):
                self.roles.append(role)
            return self.keep_take(ctx, gz, role)

        OC._c3ds_take = take
        return self

    def _wrap(self, k, fn):
        def f(*a):
            self.n[k] += 1
            return fn(*a)
        return f

    def __exit__(self, *exc):
        for k, fn in self.keep.items():
            setattr(self.OC._C, k, fn)
        self.OC._c3ds_take = self.keep_take
        return False


@pytest.mark.parametrize("w,stride", [(64, 1), (128, 2)])
def test_stage_grads_on_vs_off(cuda, tune, w, stride):
    """Downsample block + identity block at 8x8: input and parameter gradients
    against an fp64 run of the plain composition. What the fused kernel stores
    is bit-identical to the unfused path, so the error with the fusion on must
    equal the error with it off to the digits printed."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    st = _stage(cuda, w, stride)
    x, wgt = _inputs(cuda, w if stride == 1 else 2 * w, 4 * w, 8 // stride)
    gref = _ref_grads(st, x, wgt, w, stride)
    res = {}
    for mode in (1, 0):
        tune(c3bwd64=1, c3bwd128=1, c3bwd_ds64=mode, c3bwd_ds128=mode)
        with _Spy("conv3_bwd_ds_fused", "bn_bwd_apply2_g") as spy:
            res[mode] = _run_chain(copy.deepcopy(st), x, wgt)
        assert spy.n["conv3_bwd_ds_fused"] == mode and spy.n["bn_bwd_apply2_g"] == 1 - mode, spy.n
        assert sorted(spy.roles) == ([0, 1] if mode else [])
        assert not OC._C3DS_DEFERRED and not OC._C3_DEFERRED, "deferred-gradient registry not empty after backward"
    e_on, e_off = _rel(res[1], gref), _rel(res[0], gref)
    print(f"w={w} stride={stride}: gradient rel-L2 error vs fp64: fused {e_on:.3e}, unfused {e_off:.3e}")
    assert bool(torch.isfinite(res[1]).all())
    assert e_off < 0.5, e_off  # the fp64 composition is the same function (bf16 chain vs fp64)
    assert f"{e_on:.3e}" == f"{e_off:.3e}", (e_on, e_off)


def test_both_node_orders(cuda, tune):
    """Either marked node may run first; whichever does launches the kernel."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    tune(c3bwd64=1, c3bwd_ds64=1)
    st = _stage(cuda, 64)
    x, wgt = _inputs(cuda, 64, 256, 8)
    gref = _ref_grads(st, x, wgt, 64, 1)
    tune(c3bwd_ds64=0)
    e_off = _rel(_run_manual(copy.deepcopy(st), x, wgt, True), gref)
    tune(c3bwd_ds64=1)
    got, first = {}, {}
    for ds_first in (True, False):
        with _Spy("conv3_bwd_ds_fused", "conv1x1_dgrad") as spy:
            got[ds_first] = _run_manual(copy.deepcopy(st), x, wgt, ds_first)
        assert spy.n["conv3_bwd_ds_fused"] == 1, spy.n
        # block 0's conv1 node runs the one plain data gradient left
        assert spy.n["conv1x1_dgrad"] == 1, "the downsample conv still ran its own data gradient"
        assert sorted(spy.roles) == [0, 1] and not OC._C3DS_DEFERRED
        first[ds_first] = spy.roles[0]
        e = _rel(got[ds_first], gref)
        print(f"downsample conv built first={ds_first}: node {spy.roles[0]} launched, error vs fp64 {e:.3e} "
              f"(unfused {e_off:.3e})")
        assert f"{e:.3e}" == f"{e_off:.3e}", (e, e_off)
    assert first[True] != first[False], "both graphs ran the two nodes in the same order"
    # the RED sums' atomic order is the only difference between two runs
    assert _rel(got[True], got[False]) < 1e-3


def test_routing_falls_through(cuda, tune):
    """No raise and today's kernels where the fusion does not apply."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    tune(c3bwd64=1, c3bwd128=1, c3bwd_ds64=1, c3bwd_ds128=0)
    names = ("conv3_bwd_ds_fused", "bn_bwd_apply2_g")
    # stride-2 downsample convs: layer-2 style with its variant off, and w = 64 (no store-only variant there)
    for w in (128, 64):
        st = _stage(cuda, w, 2)
        x, wgt = _inputs(cuda, 2 * w, 4 * w, 4)
        with _Spy(*names) as spy:
            g = _run_chain(st, x, wgt)
        assert spy.n == {"conv3_bwd_ds_fused": 0, "bn_bwd_apply2_g": 1} and not spy.roles, (w, spy.n)
        assert bool(torch.isfinite(g).all()) and not OC._C3DS_DEFERRED
    st = _stage(cuda, 64)
    x, wgt = _inputs(cuda, 64, 256, 8)
    # c3bwd_ds=0, and c3bwd=0 which turns everything off
    for kv in (dict(c3bwd_ds64=0), dict(c3bwd_ds64=1, c3bwd64=0)):
        tune(**kv)
        with _Spy(*names) as spy:
            _run_chain(copy.deepcopy(st), x, wgt)
        assert spy.n == {"conv3_bwd_ds_fused": 0, "bn_bwd_apply2_g": 1} and not spy.roles, (kv, spy.n)
    tune(c3bwd64=1, c3bwd_ds64=1)
    # fp32 activations and eval mode: off the fused GEMM path altogether
    with _Spy(*names) as spy:
        xf = x.float().requires_grad_(True)
        (copy.deepcopy(st)(xf) * wgt).sum().backward()
        ev = copy.deepcopy(st).eval()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            xe = x.detach().requires_grad_(True)
            (ev(xe).float() * wgt).sum().backward()
    assert spy.n["conv3_bwd_ds_fused"] == 0 and not spy.roles and not OC._C3DS_DEFERRED
    assert bool(torch.isfinite(xf.grad).all()) and bool(torch.isfinite(xe.grad).all())


def test_second_consumer_of_z3_raises(cuda, tune):
    """z3 with a second consumer: autograd sums the gradients, the conv3 node
    does not get the boundary's deferred gradient and must refuse it."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    tune(c3bwd64=1, c3bwd_ds64=1)
    st = _stage(cuda, 64)
    x, wgt = _inputs(cuda, 64, 256, 8)
    with pytest.raises(RuntimeError, match="conv3 backward fusion.*c3bwd_ds=0"):
        _run_manual(st, x, wgt, True, extra_consumer=True)
    assert not OC._C3DS_DEFERRED and not OC._C3_DEFERRED


def test_untaken_entry_raises_at_next_boundary(cuda, tune):
    from distributed_compute_pytorch_amd.ops import conv as OC

    g = torch.zeros(1, 256, 2, 2, device=cuda, dtype=torch.bfloat16)
    OC._c3ds_put(g, (None,) * 10, (None, None, True))
    with pytest.raises(RuntimeError, match="never taken.*c3bwd_ds=0"):
        OC._c3_put(g, None, None, None, None, None)
    assert not OC._C3DS_DEFERRED and not OC._C3_DEFERRED
    OC._c3ds_put(g, (None,) * 10, (None, None, True))
    OC._C3DS_DEFERRED[g.data_ptr()].taken.add(0)
    with pytest.raises(RuntimeError, match="only one of its two nodes.*c3bwd_ds=0"):
        OC._c3ds_put(g, (None,) * 10, (None, None, True))
    assert not OC._C3DS_DEFERRED


def test_fused_backward_replays_in_hip_graph(cuda, tune):
    """Forward + backward of the stage captured once and replayed on a new
    input: gradients equal an eager run on the same input, and the registry
    holds nothing after capture or replay."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    tune(c3bwd64=1, c3bwd_ds64=1)
    st = _stage(cuda, 64, seed=3)
    eager = copy.deepcopy(st)
    xs, wgt = _inputs(cuda, 64, 256, 8, seed=11)
    xn, _ = _inputs(cuda, 64, 256, 8, seed=12)

    def step():
        for p in st.parameters():
            p.grad = None
        blocks = list(st)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            h, a, head = xs, None, None
            for i, blk in enumerate(blocks):
                h, a, head = blk.chain(h, a, head, blocks[i + 1] if i + 1 < len(blocks) else None)
            (h.float() * wgt).sum().backward()
        return [p.grad for p in st.parameters()]

    xs.requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grads = step()
    assert not OC._C3DS_DEFERRED, "registry holds tensors after capture"
    with torch.no_grad():
        xs.copy_(xn)
    graph.replay()
    torch.cuda.synchronize()
    assert not OC._C3DS_DEFERRED
    got = torch.cat([xs.grad.double().reshape(-1)] + [g.double().reshape(-1) for g in grads])
    want = _run_chain(eager, xn, wgt)
    assert bool(torch.isfinite(got).all())
    # atomics order is the only difference between a replay and an eager run
    assert _rel(got, want) < 1e-2, _rel(got, want)
