"""Achieved HBM bandwidth of the hand-written kernels on the shapes the
workloads run (ResNet-50 b256 BN / max-pool, GPT-2 LayerNorm / cross-entropy
/ dropout, optimizer updates over a full model).

Bytes are the analytic minimum each op must move (every input read once,
every output written once); time is HIP-event time over `--iters` calls.
Run under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` for counter
evidence (gfx950 FETCH_SIZE reads half of a streaming read's bytes).

    python tools/kernel_bench.py [--iters 20] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import distributed_compute_pytorch_amd as dcp  # noqa: E402
from distributed_compute_pytorch_amd._ext import C as _C  # noqa: E402


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def llama_ops(rec, iters, dev):
    """RMSNorm / RoPE / SwiGLU kernels next to the stock PyTorch composition of
    each op (back to back, same tensors) and, as the yardstick on the same
    box, the LayerNorm kernels at the same shapes. Bytes: the analytic minimum
    of the fused op (RMSNorm fwd bf16 4 B/elem; SwiGLU fwd 6 B per output
    element; RoPE in place 2 × 2/3 of the packed bytes), also charged to the
    stock rows so their TB/s reads as "effective"."""
    from distributed_compute_pytorch_amd.ops.rope import rope_qkv_reference, rope_table

    bf = torch.bfloat16

    def stock_rms(x, w):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6) * w).to(x.dtype)

    for rows, D in [(8192, 768), (16384, 1024)]:
        x = torch.randn(rows, D, device=dev).to(bf)
        w, b = torch.rand(D, device=dev) + 0.5, torch.zeros(D, device=dev)
        dy = torch.randn(rows, D, device=dev).to(bf)
        E = rows * D
        _, rstd = _C.rms_norm_fwd(x, w, 1e-6)
        rec(f"rmsnorm fwd bf16 [{rows},{D}]", timeit(lambda: _C.rms_norm_fwd(x, w, 1e-6), iters), E * 4)
        rec(f"rmsnorm bwd bf16 [{rows},{D}]", timeit(lambda: _C.rms_norm_bwd(dy, x, w, rstd), iters), E * 6)
        _, mu, rs = _C.layer_norm_fwd(x, w, b, 1e-5, bf)
        rec(f"layernorm fwd bf16 [{rows},{D}] (yardstick)", timeit(lambda: _C.layer_norm_fwd(x, w, b, 1e-5, bf), iters),
            E * 4)
        rec(f"layernorm bwd bf16 [{rows},{D}] (yardstick)",
            timeit(lambda: _C.layer_norm_bwd(dy, x, w, b, mu, rs), iters), E * 6)
        rec(f"stock rmsnorm fwd bf16 [{rows},{D}]", timeit(lambda: stock_rms(x, w), iters), E * 4)
        xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()

        def stock_fb():
            xr.grad = wr.grad = None
            stock_rms(xr, wr).backward(dy)

        rec(f"stock rmsnorm fwd+bwd bf16 [{rows},{D}]", timeit(stock_fb, iters), E * 10)

    B, T, C3, H = 8, 1024, 2304, 12
    table = rope_table(T, 10000.0, dev)
    qkv = torch.randn(B, T, C3, device=dev).to(bf)
    nb = qkv.numel() * 2
    rec(f"rope in place [{B},{T},{C3}]", timeit(lambda: _C.rope_qkv(qkv, H, table, False, True), iters), nb * 4 // 3)
    rec(f"rope out of place (the backward) [{B},{T},{C3}]",
        timeit(lambda: _C.rope_qkv(qkv, H, table, True, False), iters), nb * 2)
    rec(f"stock rope [{B},{T},{C3}]", timeit(lambda: rope_qkv_reference(qkv, H, table), iters), nb * 4 // 3)

    M, Fh = 8192, 2048
    p = torch.randn(M, 2 * Fh, device=dev).to(bf)
    dy = torch.randn(M, Fh, device=dev).to(bf)
    rec(f"swiglu fwd [{M},2*{Fh}]", timeit(lambda: _C.swiglu_fwd(p), iters), M * Fh * 6)
    rec(f"swiglu bwd [{M},2*{Fh}]", timeit(lambda: _C.swiglu_bwd(dy, p), iters), M * Fh * 10)

    def stock_swiglu(t):
        g, u = t.chunk(2, -1)
        return F.silu(g) * u

    rec(f"stock swiglu fwd [{M},2*{Fh}]", timeit(lambda: stock_swiglu(p), iters), M * Fh * 6)
    pr = p.clone().requires_grad_()

    def stock_swiglu_fb():
        pr.grad = None
        stock_swiglu(pr).backward(dy)

    rec(f"stock swiglu fwd+bwd [{M},2*{Fh}]", timeit(stock_swiglu_fb, iters), M * Fh * 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, choices=["llama"], help="run one section only")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    res = []

    def rec(name, ms, nbytes):
        r = {"op": name, "us": round(ms * 1e3, 1), "GB": round(nbytes / 1e9, 3),
             "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 2)}
        res.append(r)
        print(json.dumps(r), flush=True)

    if a.only == "llama":
        llama_ops(rec, a.iters, dev)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return

    cl = torch.channels_last
    for (n, c, h, w, resid) in [(256, 64, 56, 56, False), (256, 256, 56, 56, True), (256, 128, 28, 28, False),
                                (256, 1024, 14, 14, True), (256, 512, 7, 7, False)]:
        x = torch.randn(n, c, h, w, device=dev).to(bf).contiguous(memory_format=cl)
        r = torch.randn_like(x) if resid else None
        wgt, b = torch.ones(c, device=dev), torch.zeros(c, device=dev)
        rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        E = x.numel() * 2
        out = {}

        def fwd():
            out["o"] = _C.bn_act_fwd(x, wgt, b, rm, rv, r, True, 0.1, 1e-5, True)

        ms = timeit(fwd, a.iters)
        rec(f"bn_fwd{'+res' if resid else ''}+relu [{n},{c},{h},{w}] (stats + apply)", ms, E * (3 + (1 if resid else 0)))
        y, mean, invstd, bits = out["o"]
        gy = torch.randn_like(x)
        gy2 = torch.randn_like(x) if resid else None

        def bwd():
            _C.bn_act_bwd(gy, gy2, x, wgt, b, mean, invstd, y, True, resid, True, bits if resid else None)

        ms = timeit(bwd, a.iters)
        # reduce: gy (+gy2) + x (+bits) [+ write g]; apply: g + x → dx
        nb = E * (2 + (1 if resid else 0)) + (E // 16 if resid else 0) + (E if resid else 0) + E * 3
        rec(f"bn_bwd{'+res(dual)' if resid else ''}+relu [{n},{c},{h},{w}] (reduce + apply)", ms, nb)

    x = torch.randn(256, 64, 112, 112, device=dev).to(bf).contiguous(memory_format=cl)
    out = {}
    ms = timeit(lambda: out.__setitem__("o", _C.maxpool2d_fwd(x, 3, 2, 1)), a.iters)
    yo, idx = out["o"]
    rec("maxpool3x3s2 fwd [256,64,112,112]", ms, x.numel() * 2 + yo.numel() * 3)
    gy = torch.randn_like(yo)
    ms = timeit(lambda: _C.maxpool2d_bwd(gy, idx, list(x.shape), 3, 2, 1), a.iters)
    rec("maxpool3x3s2 bwd [256,64,112,112]", ms, gy.numel() * 3 + x.numel() * 2)

    T, D, V = 8 * 1024, 768, 50257
    xf = torch.randn(T, D, device=dev)
    lw, lb = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    out = {}
    ms = timeit(lambda: out.__setitem__("o", _C.layer_norm_fwd(xf, lw, lb, 1e-5, bf)), a.iters)
    rec(f"layernorm fwd fp32->bf16 [{T},{D}]", ms, T * D * (4 + 2))
    yl, mu, rs = out["o"]
    dy = torch.randn(T, D, device=dev).to(bf)
    ms = timeit(lambda: _C.layer_norm_bwd(dy, xf, lw, lb, mu, rs), a.iters)
    rec(f"layernorm bwd [{T},{D}]", ms, T * D * (2 + 4 + 4))

    xb = torch.randn(2 * T, D, device=dev).to(bf)
    ms = timeit(lambda: out.__setitem__("o", _C.layer_norm_fwd(xb, lw, lb, 1e-5, bf)), a.iters)
    rec(f"layernorm fwd bf16 [{2 * T},{D}]", ms, 2 * T * D * (2 + 2))
    yl, mu, rs = out["o"]
    dyb = torch.randn(2 * T, D, device=dev).to(bf)
    ms = timeit(lambda: _C.layer_norm_bwd(dyb, xb, lw, lb, mu, rs), a.iters)
    rec(f"layernorm bwd bf16 [{2 * T},{D}]", ms, 2 * T * D * (2 + 2 + 2))

    logits = torch.randn(T, V, device=dev).to(bf)
    tgt = torch.randint(0, V, (T,), device=dev)
    out = {}
    ms = timeit(lambda: out.__setitem__("o", _C.cross_entropy_fwd(logits, tgt, -100, 0.0)), a.iters)
    rec(f"softmax-xent fwd [{T},{V}] bf16", ms, logits.numel() * 2)
    loss, lse = out["o"]
    dl = torch.full((1,), 1.0 / T, device=dev)
    ms = timeit(lambda: _C.cross_entropy_bwd(logits, tgt, lse, dl, -100, 0.0), a.iters)
    rec(f"softmax-xent bwd [{T},{V}] bf16", ms, logits.numel() * 4)

    xd = torch.randn(T * D * 4, device=dev).to(bf)
    rd = torch.randn_like(xd)
    ms = timeit(lambda: _C.dropout_fwd(xd, rd, 0.1, 1234, 0), a.iters)
    rec(f"dropout+residual [{T * D * 4}] bf16", ms, xd.numel() * 6)

    from distributed_compute_pytorch_amd.models import gpt2_small, resnet50

    for name, m, kind in [("resnet50", resnet50(), "sgd"), ("gpt2-small", gpt2_small(), "adamw")]:
        ps = [p.detach().to(dev) for p in m.parameters()]
        gs = [torch.randn_like(p) for p in ps]
        nel = sum(p.numel() for p in ps)
        if kind == "sgd":
            bufs = [torch.zeros_like(p) for p in ps]
            ms = timeit(lambda: _C.fused_sgd(ps, gs, bufs, 0.1, 0.9, 0.0, 1e-4, False, False, False, 1.0), a.iters)
            rec(f"fused SGD-momentum {name} ({nel / 1e6:.1f}M params, one launch)", ms, nel * 4 * 5)
        else:
            opt = dcp.optim.AdamW([torch.nn.Parameter(p) for p in ps], lr=1e-4)
            for p, g in zip(opt.param_groups[0]["params"], gs):
                p.grad = g
            ms = timeit(lambda: opt.step(), a.iters)
            rec(f"fused AdamW {name} ({nel / 1e6:.1f}M params, one launch)", ms, nel * 4 * 7)
        del m

    # Layer-wise optimizers next to the elementwise ones they replace at large
    # batch, on the same parameter lists and back to back: LAMB vs AdamW over
    # BERT-base, LARS vs SGD over ResNet-50. "op" rows time the bare _C call
    # (GPU time of the launches), "step" rows the optimizer's step() with its
    # host work. Bytes: AdamW 7 and LAMB 11 fp32 words per parameter (LAMB's
    # norm pass reads p, g, m, v once more); SGD 5 and LARS 7 (p, g again).
    from distributed_compute_pytorch_amd.models import bert_base

    def no_decay_split(ps):
        return [{"params": [p for p in ps if p.ndim > 1]},
                {"params": [p for p in ps if p.ndim <= 1], "weight_decay": 0.0}]

    for name, m, pair in [("bert-base", bert_base(), ("AdamW", "LAMB")), ("resnet50", resnet50(), ("SGD", "LARS"))]:
        ps = [torch.nn.Parameter(p.detach().to(dev)) for p in m.parameters()]
        del m
        for p in ps:
            p.grad = torch.randn_like(p)
        gs = [p.grad for p in ps]
        nel = sum(p.numel() for p in ps)
        tag = f"{name} ({nel / 1e6:.1f}M params)"
        s1 = [torch.zeros_like(p) for p in ps]
        s2 = [torch.zeros_like(p) for p in ps]
        if pair[1] == "LAMB":
            ops = [("AdamW", 7, lambda: _C.fused_adam(ps, gs, s1, s2, [], 1e-4, 0.9, 0.999, 1e-8, 0.01, 10.0, False,
                                                      True, False, 1.0)),
                   ("LAMB", 11, lambda: _C.fused_lamb(ps, gs, s1, s2, 1e-4, 0.9, 0.999, 1e-6, 0.01, 10.0, True, False,
                                                      False, 1.0))]
            opts = [("AdamW", 7, dcp.optim.AdamW(no_decay_split(ps), lr=1e-4, weight_decay=0.01)),
                    ("LAMB", 11, dcp.optim.LAMB(no_decay_split(ps), lr=1e-4, weight_decay=0.01))]
        else:
            ops = [("SGD-momentum", 5, lambda: _C.fused_sgd(ps, gs, s1, 0.1, 0.9, 0.0, 1e-4, False, False, False,
                                                            1.0)),
                   ("LARS", 7, lambda: _C.fused_lars(ps, gs, s1, 0.1, 0.9, 0.0, 1e-4, False, False, False, 1e-3, 1e-8,
                                                     False, 1.0))]
            opts = [("SGD-momentum", 5, dcp.optim.SGD(no_decay_split(ps), lr=0.1, momentum=0.9, weight_decay=1e-4)),
                    ("LARS", 7, dcp.optim.LARS(no_decay_split(ps), lr=0.1, momentum=0.9, weight_decay=1e-4))]
        for label, words, fn in ops:
            rec(f"fused {label} op {tag}", timeit(fn, a.iters), nel * 4 * words)
        for label, words, opt in opts:
            rec(f"fused {label} step {tag}", timeit(lambda: opt.step(), a.iters), nel * 4 * words)
    llama_ops(rec, a.iters, dev)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
