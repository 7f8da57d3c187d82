"""Block boundary forward with the next block's conv1 fed from the tile that
forms y (csrc/kernels/conv1_fwd.hip, `_C.conv1_fwd_fused`) against the
unfused composition `bn_act_fwd` / `bn_resbn_act_fwd` -> `conv1x1_fwd`
(`gemm_tune c1fwd=0`), both through `ops.conv.bn_res_act_conv1x1`.

y, its mask bits, both BNs' mean / invstd, the running statistics and
num_batches_tracked must match bit for bit, and so must z1: the kernel feeds
the MFMAs the same y bits in gemm_nt's k order. (Σz1, Σz1²): oracle = fp64
torch on the same bf16 operands — z1 from the bf16 y, the sums from the
bf16-rounded oracle z1; metric = relative L2 norm ‖a − o‖ / ‖o‖; the fused
path must stay within 1.5x the unfused path's error measured in the same test
(only the fp32 accumulation / atomic order differs).

Tiles are 32 rows: 25 rows = less than one tile, 50 = one tile + a ragged
tail, 162 = five tiles + a 2-row tail; `c1fwd_grid` = 2 makes each workgroup
run three tiles, so the register prefetch crosses tile boundaries.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

MARGIN = 1.5
KEYS = ("c1fwd64", "c1fwd128", "c1fwd256x128", "c1fwd_grid")


def _rel(a, o):
    return float((a.double() - o).norm() / o.norm().clamp_min(1e-30))


@pytest.fixture()
def tune():
    from distributed_compute_pytorch_amd import _C

    old = {k: _C.gemm_tune_get(k) for k in KEYS}

    def set_(**kv):
        for k, v in kv.items():
            _C.gemm_tune(k, v)

    yield set_
    for k, v in old.items():
        _C.gemm_tune(k, v)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _bn(dev, C, gen):
    bn = torch.nn.BatchNorm2d(C).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(C, generator=gen) * 0.3 + 1)
        bn.bias.copy_(torch.randn(C, generator=gen) * 0.2)
        bn.running_mean.copy_(torch.randn(C, generator=gen) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=gen) + 0.5)
    return bn


def _sums(t):
    """(Σx, Σx²) fp32 [2C] of a bf16 NHWC tensor, as a GEMM epilogue hands them over."""
    r = _rows(t).double()
    return torch.cat([r.sum(0), (r * r).sum(0)]).float().contiguous()


def _case(dev, K, Nout, N, hw, rbn):
    gen = torch.Generator(device="cpu").manual_seed(100 * K + Nout + 10 * N * hw + int(rbn))
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    cl = lambda t: t.to(dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)  # noqa: E731
    z3 = cl(r(N, K, hw, hw) * 1.5 + 0.3)
    res = cl(r(N, K, hw, hw) * (2.0 if rbn else 1.0) - (0.4 if rbn else 0.0))
    w = (r(Nout, K, 1, 1) * (K ** -0.5)).to(dev)
    return dict(z3=z3, res=res, w=w, bn3=_bn(dev, K, gen), bnd=_bn(dev, K, gen) if rbn else None,
                s3=_sums(z3), sd=_sums(res) if rbn else None)


_CASES = {}


def _cached_case(dev, *key):
    if key not in _CASES:
        _CASES[key] = _case(dev, *key)
    return _CASES[key]


def _boundary(c):
    """One `bn_res_act_conv1x1` call on fresh copies of the case's BNs: every
    tensor the node returns or saves, and the BN buffers afterwards."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    bn3, bnd = copy.deepcopy(c["bn3"]), copy.deepcopy(c["bnd"])
    z3 = c["z3"].clone().requires_grad_()
    if bnd is not None:
        y, z1, s1 = OC.bn_res_act_conv1x1(bn3, z3, c["s3"].clone(), None, c["w"], (bnd, c["res"], c["sd"].clone()))
    else:
        y, z1, s1 = OC.bn_res_act_conv1x1(bn3, z3, c["s3"].clone(), c["res"], c["w"])
    _, _, mean, invstd, bits, ysaved, _, _, _, mean2, invstd2 = y.grad_fn.saved_tensors
    assert ysaved.data_ptr() == y.data_ptr()
    out = dict(y=y.detach(), z1=z1.detach(), s1=s1.clone(), bits=bits, mean=mean, invstd=invstd,
               rm=bn3.running_mean, rv=bn3.running_var, nbt=bn3.num_batches_tracked)
    if bnd is not None:
        out.update(mean2=mean2, invstd2=invstd2, rm2=bnd.running_mean, rv2=bnd.running_var,
                   nbt2=bnd.num_batches_tracked)
    return out


def _counting(monkeypatch):
    """Counts `_C.conv1_fwd_fused` calls made by ops.conv; returns the counter."""
    from distributed_compute_pytorch_amd.ops import conv as OC

    calls = {"n": 0, "rbn": 0}
    real = OC._C.conv1_fwd_fused

    def counted(*a, **kw):
        calls["n"] += 1
        calls["rbn"] += int(len(a) > 11 and a[11] is not None)
        return real(*a, **kw)

    monkeypatch.setattr(OC._C, "conv1_fwd_fused", counted)
    return calls


SHAPES = [(256, 64, False), (256, 64, True), (512, 128, False), (512, 128, True), (256, 128, False)]


@pytest.mark.parametrize("grid", [0, 2])
@pytest.mark.parametrize("N,hw", [(1, 5), (2, 5), (2, 9)])
@pytest.mark.parametrize("K,Nout,rbn", SHAPES)
def test_fused_matches_unfused(cuda, tune, monkeypatch, K, Nout, rbn, N, hw, grid):
    from distributed_compute_pytorch_amd import _C

    M = N * hw * hw
    if grid and M <= 64:
        grid = 1  # small cases: one workgroup runs every tile
    c = _cached_case(cuda, K, Nout, N, hw, rbn)
    calls = _counting(monkeypatch)
    tune(c1fwd64=1, c1fwd128=1, c1fwd256x128=1, c1fwd_grid=grid)
    assert _C.conv1_fwd_mode(M, K, Nout) == 1
    f = _boundary(c)
    assert calls["n"] == 1 and calls["rbn"] == int(rbn), "the fused boundary did not run"
    tune(c1fwd64=0, c1fwd128=0, c1fwd256x128=0)
    assert _C.conv1_fwd_mode(M, K, Nout) == 0
    u = _boundary(c)
    assert calls["n"] == 1, "c1fwd=0 still ran the fused boundary"
    torch.cuda.synchronize()
    exact = ["y", "bits", "mean", "invstd", "rm", "rv", "nbt"] + (["mean2", "invstd2", "rm2", "rv2", "nbt2"] if rbn else [])
    for k in exact:
        assert f[k].shape == u[k].shape and torch.equal(f[k], u[k]), f"{k} differs from the unfused path's"
    assert int(f["nbt"]) == 1
    assert f["z1"].shape == u["z1"].shape and f["z1"].is_contiguous(memory_format=torch.channels_last)
    # the mask is y's sign and not everything is masked
    yr = _rows(f["y"])
    bits = ((f["bits"].view(M, K // 8, 1) >> torch.arange(8, device=cuda).view(1, 1, 8)) & 1).reshape(M, K)
    assert torch.equal(bits.bool(), yr > 0) and 0.2 < float((yr > 0).float().mean()) < 0.9
    # ---- fp64 oracle from the bf16 y
    z1_o = yr.double() @ c["w"].view(Nout, K).to(torch.bfloat16).double().t()
    zb = z1_o.to(torch.bfloat16).double()
    s1_o = torch.cat([zb.sum(0), (zb * zb).sum(0)])
    # same y bits and the same MFMA k order as gemm_nt: z1 is bit-identical; the
    # sums are held to the margin
    same = torch.equal(f["z1"], u["z1"])
    errs = {
        "z1": (_rel(_rows(f["z1"]), z1_o), _rel(_rows(u["z1"]), z1_o)),
        "sum": (_rel(f["s1"][:Nout], s1_o[:Nout]), _rel(u["s1"][:Nout], s1_o[:Nout])),
        "sumsq": (_rel(f["s1"][Nout:], s1_o[Nout:]), _rel(u["s1"][Nout:], s1_o[Nout:])),
    }
    print(f"K={K} N={Nout} rbn={rbn} M={M} grid={grid} z1 bit-identical={same}; (fused, unfused) rel-L2 errors: "
          + ", ".join(f"{k}=({a:.3e}, {b:.3e})" for k, (a, b) in errs.items()))
    assert same, "z1 differs from gemm_nt's"
    for k, (ef, eu) in errs.items():
        assert ef <= MARGIN * eu, (k, ef, eu)
    # the unfused error itself is bf16 rounding of the output, not garbage
    assert errs["z1"][1] < 1e-2 and errs["sum"][1] < 1e-3 and errs["sumsq"][1] < 1e-3


def _stage(dev, w, rbn, fused=True, seed=0):
    """Two bottlenecks whose boundary is an identity one (both blocks identity)
    or an RBN one (block 0 has a stride-1 downsample branch, as layer1's)."""
    from distributed_compute_pytorch_amd.models import resnet as R

    torch.manual_seed(seed)
    if rbn:
        cin = w
        b0 = R.Bottleneck(cin, w, 1, R._downsample(cin, 4 * w, 1, fused), fused_bn=fused)
    else:
        cin = 4 * w
        b0 = R.Bottleneck(cin, w, fused_bn=fused)
    st = R.BottleneckStage(b0, R.Bottleneck(4 * w, w, fused_bn=fused))
    for m in st.modules():
        if hasattr(m, "running_mean") and getattr(m, "weight", None) is not None:
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, 0.0, 0.2)
    return st.to(dev).to(memory_format=torch.channels_last).train(), cin


def _run_chain(st, x, wgt, backward=True):
    """The stage's blocks as ResNet._chain runs them (block 0's BN3 fused into
    block 1's conv1 node); returns the parameter gradients (or the output)."""
    blocks = list(st)
    for p in st.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h, a, head = x, None, None
        for i, blk in enumerate(blocks):
            h, a, head = blk.chain(h, a, head, blocks[i + 1] if i + 1 < len(blocks) else None)
        if not backward:
            return h
        loss = (h.float() * wgt).sum()
    loss.backward()
    return [p.grad for p in st.parameters()]


@pytest.mark.parametrize("w,rbn", [(64, False), (64, True), (128, False), (128, True)])
def test_stage_param_grads_on_vs_off(cuda, tune, monkeypatch, w, rbn):
    """Two bottlenecks at 8x8 around an identity / RBN boundary: parameter
    gradients with the fused boundary on and off against an fp64 run of the
    plain composition; on must stay within 1.5x off's error (relative L2 over
    all parameters)."""
    st, cin = _stage(cuda, w, rbn)
    gen = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(4, cin, 8, 8, generator=gen).to(cuda).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    wgt = torch.randn(4, 4 * w, 8, 8, generator=gen).to(cuda)
    ref, _ = _stage(cuda, w, rbn, fused=False)
    ref.load_state_dict(st.state_dict())
    ref = ref.double().train()
    (ref(x.double()) * wgt.double()).sum().backward()
    gref = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])

    calls = _counting(monkeypatch)
    res, bufs = {}, {}
    for mode in (1, 0):
        tune(c1fwd64=mode, c1fwd128=mode, c1fwd256x128=mode)
        m = copy.deepcopy(st)
        calls["n"] = calls["rbn"] = 0
        grads = _run_chain(m, x, wgt)
        assert calls["n"] == (1 if mode else 0), "the fused boundary did not run exactly where it should"
        assert calls["rbn"] == (int(rbn) if mode else 0)
        res[mode] = torch.cat([g.double().reshape(-1) for g in grads])
        bufs[mode] = [b.clone() for b in m.buffers()]
    e_on, e_off = _rel(res[1], gref), _rel(res[0], gref)
    print(f"w={w} rbn={rbn}: parameter-gradient rel-L2 error vs fp64: fused {e_on:.3e}, unfused {e_off:.3e}")
    assert bool(torch.isfinite(res[1]).all())
    assert e_off < 0.5, e_off  # the fp64 composition is the same function (bf16 chain vs fp64: ~0.13 at 256 rows)
    assert e_on <= MARGIN * e_off, (e_on, e_off)
    # the boundary's own BNs (block 0's bn3 / downsample BN) publish bit-identical buffers
    names = [n for n, _ in st.named_buffers()]
    for n, a, b in zip(names, bufs[1], bufs[0]):
        if n.startswith("0.bn3.") or n.startswith("0.downsample."):
            assert torch.equal(a, b), n


def test_routing_keeps_the_old_path(cuda, tune, monkeypatch):
    """K = 1024 (not a covered shape), an eval-mode stage and RES_PROLOGUE all
    stay off the fused boundary; the covered shape next to them takes it."""
    from distributed_compute_pytorch_amd.models import resnet as R
    from distributed_compute_pytorch_amd.ops import conv as OC

    tune(c1fwd64=1, c1fwd128=1, c1fwd256x128=1)
    calls = _counting(monkeypatch)
    from distributed_compute_pytorch_amd import _C

    mk = lambda c: torch.randn(2, c, 8, 8, device=cuda).to(torch.bfloat16).contiguous(  # noqa: E731
        memory_format=torch.channels_last)
    assert _C.conv1_fwd_mode(128, 1024, 256) == 0 and _C.conv1_fwd_mode(128, 256, 64) == 1
    wide = R.BottleneckStage(R.Bottleneck(1024, 256, fused_bn=True), R.Bottleneck(1024, 256, fused_bn=True))
    wide = wide.to(cuda).to(memory_format=torch.channels_last).train()
    _run_chain(wide, mk(1024), None, backward=False)
    assert calls["n"] == 0, "K = 1024 took the fused boundary"
    st, _ = _stage(cuda, 64, False)
    _run_chain(st, mk(256), None, backward=False)
    assert calls["n"] == 1, "the covered shape did not take the fused boundary"
    with torch.no_grad():
        _run_chain(copy.deepcopy(st).eval(), mk(256), None, backward=False)
    assert calls["n"] == 1, "an eval-mode stage took the fused boundary"
    monkeypatch.setattr(OC, "RES_PROLOGUE", True)
    _run_chain(st, mk(256), None, backward=False)
    assert calls["n"] == 1, "RES_PROLOGUE did not keep the GEMM-prologue path"
    # layer1 -> layer2: conv1 of 256 -> 128 channels behind an identity block
    monkeypatch.setattr(OC, "RES_PROLOGUE", False)
    x21 = R.BottleneckStage(R.Bottleneck(256, 64, fused_bn=True),
                            R.Bottleneck(256, 128, 1, R._downsample(256, 512, 1, True), fused_bn=True))
    x21 = x21.to(cuda).to(memory_format=torch.channels_last).train()
    _run_chain(x21, mk(256), None, backward=False)
    assert calls["n"] == 2 and calls["rbn"] == 0
    torch.cuda.synchronize()


def test_fused_boundary_replays_in_hip_graph(cuda, tune):
    """Forward + backward of the two-block chain captured once and replayed on
    new inputs: gradients equal an eager run on the same inputs."""
    tune(c1fwd64=1)
    st, _ = _stage(cuda, 64, True, seed=3)
    eager = copy.deepcopy(st)
    gen = torch.Generator(device="cpu").manual_seed(11)
    mk = lambda: torch.randn(4, 64, 8, 8, generator=gen).to(cuda).to(torch.bfloat16).contiguous(  # noqa: E731
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
    for _ in range(2):
        xn = mk()
        xs.copy_(xn)
        graph.replay()
        torch.cuda.synchronize()
        # BN running statistics do not enter training-mode gradients: a fresh copy is an equal model
        want = _run_chain(copy.deepcopy(eager), xn, wgt)
        got = torch.cat([g.double().reshape(-1) for g in grads])
        exp = torch.cat([g.double().reshape(-1) for g in want])
        assert bool(torch.isfinite(got).all())
        # atomics order is the only difference between a replay and an eager run
        assert _rel(got, exp) < 1e-2, _rel(got, exp)
