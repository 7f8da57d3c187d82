"""Fused against unfused conv3 backward of a downsample block at the real
ResNet-50 shapes (1,024 and 37 images at 56x56, w = 64; 1,024 images at 28x28,
w = 128): `_C.conv3_bwd_ds_fused` against `bn_bwd_apply2_g` ->
`conv1x1_dgrad_bnred` / `conv1x1_dgrad` on random operands. Prints whether
dz3, dzd, dy2 and dx_d are bit-identical and the relative difference of the
RED sums (fp32 atomics in both paths); exit status 1 if a stored tensor
differs. Needs about 12 GB of device memory.

    python tools/c3ds_realshape.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from distributed_compute_pytorch_amd import _C
dev = torch.device("cuda", 0)
torch.manual_seed(0)
def run(w, N, hw):
    C = 4 * w
    cl = lambda *s: torch.randn(*s, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    z3, zd, x2 = cl(N, C, hw, hw), cl(N, C, hw, hw), cl(N, w, hw, hw)
    g = (torch.randn(N, C, hw, hw, device=dev) * 0.1 * (torch.rand(N, C, hw, hw, device=dev) > 0.5)).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    M = N * hw * hw
    f = lambda n, s=1.0, o=0.0: (torch.randn(n, device=dev) * s + o).contiguous()
    wt = (torch.randn(w, C, device=dev) * C ** -0.5).to(torch.bfloat16).contiguous()
    wdt = (torch.randn(w, C, device=dev) * C ** -0.5).to(torch.bfloat16).contiguous()
    gamma3, mean3, invstd3, acc3 = f(C, .3, 1), f(C, .1), f(C, .1, 1).abs(), f(2 * C, M ** .5)
    gammad, meand, invstdd, accd = f(C, .3, 1), f(C, .1), f(C, .1, 1).abs(), f(2 * C, M ** .5)
    gamma2, beta2, mean2, invstd2 = f(w, .3, 1), f(w, .2), f(w, .1), f(w, .1, 1).abs()
    dz3, dg3, db3, dzd, dgd, dbd = _C.bn_bwd_apply2_g(g, z3, gamma3, mean3, invstd3, acc3, zd, gammad, meand, invstdd, accd)
    dy, acc2 = _C.conv1x1_dgrad_bnred(dz3, wt, x2, gamma2, beta2, mean2, invstd2)
    dxd = _C.conv1x1_dgrad(dzd, wdt) if w == 64 else None
    out = _C.conv3_bwd_ds_fused(g, z3, gamma3, mean3, invstd3, acc3, zd, gammad, meand, invstdd, accd, wt, wdt if w == 64 else None, x2, gamma2, beta2, mean2, invstd2)
    torch.cuda.synchronize()
    r = dict(dz3=torch.equal(out[2], dz3), dzd=torch.equal(out[3], dzd), dy=torch.equal(out[0], dy))
    if w == 64: r["dxd"] = torch.equal(out[4], dxd)
    r["acc2_rel"] = float((out[1].double() - acc2.double()).norm() / acc2.double().norm())
    print(f"w={w} M={M}", r, flush=True)
    return all(v for k, v in r.items() if k != "acc2_rel")
_C.gemm_tune("c3bwd_ds", 1)
ok = run(64, 1024, 56) & run(64, 37, 56) & run(128, 1024, 28)
sys.exit(0 if ok else 1)
