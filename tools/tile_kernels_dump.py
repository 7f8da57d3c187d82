"""sha256 of everything the two row-tile kernels return (csrc/kernels/conv3_bwd.hip,
conv1_fwd.hip), to compare two builds bit for bit:

    python tools/tile_kernels_dump.py > profiles/NAME.txt

Operands come from the case builders of tests/test_gpu_conv3_bwd_fused.py and
tests/test_gpu_conv1_fwd_fused.py at 25 / 50 / 162 rows (less than one 32-row
tile, one tile + a ragged tail, five tiles + a 2-row tail); `_C.conv3_bwd_fused`
/ `_C.conv1_fwd_fused` are called directly for every kernel instantiation.

Grid cap 1 (`c3bwd_grid` / `c1fwd_grid`): one workgroup runs every tile, its
float atomics land on distinct addresses in a fixed order, so the statistics
are deterministic and hashed too. Grid cap 2: only the tensors that do not come
from cross-workgroup atomics are hashed; for the statistics the line gives
max|s − s_grid1| / max|s_grid1| instead.
"""
import copy
import hashlib
import importlib.util
import os
import sys

import torch

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)

SHAPES = [(1, 5), (2, 5), (2, 9)]  # (images, height = width): 25 / 50 / 162 rows


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(R, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _report(tag, runs, stats_key):
    """runs: {grid: {name: tensor}}; one line per tensor."""
    for grid, out in runs.items():
        for k, t in out.items():
            if k == stats_key and grid != 1:
                ref = runs[1][k].double()
                d = float((t.double() - ref).abs().max() / ref.abs().max())
                print(f"{tag} grid={grid} {k} maxreldiff_vs_grid1={d:.3e}")
            else:
                print(f"{tag} grid={grid} {k} sha256={_sha(t)}")


def main():
    from distributed_compute_pytorch_amd import _C

    dev = torch.device("cuda", 0)
    t3, t1 = _load("test_gpu_conv3_bwd_fused"), _load("test_gpu_conv1_fwd_fused")
    keys = ("c3bwd64", "c3bwd128", "c3bwd_grid", "c1fwd64", "c1fwd128", "c1fwd256x128", "c1fwd_grid")
    old = {k: _C.gemm_tune_get(k) for k in keys}
    for k in keys:
        _C.gemm_tune(k, 1)
    try:
        for w in (64, 128):
            for N, hw in SHAPES:
                o, _, M = t3._case(dev, w, N, hw, False)
                runs = {}
                for grid in (1, 2):
                    _C.gemm_tune("c3bwd_grid", grid)
                    dy2, acc2, dz3 = _C.conv3_bwd_fused(o["g"], o["z3"], o["gamma3"], o["mean3"], o["invstd3"],
                                                        o["acc3"], o["wt"], o["x2"], o["gamma2"], o["beta2"],
                                                        o["mean2"], o["invstd2"])
                    torch.cuda.synchronize()
                    runs[grid] = dict(dz3=dz3, dy2=dy2, acc2=acc2)
                _report(f"conv3_bwd w={w} M={M}", runs, "acc2")
        for K, Nout in ((256, 64), (512, 128), (256, 128)):
            for rbn in (False, True):
                for N, hw in SHAPES:
                    c = t1._case(dev, K, Nout, N, hw, rbn)
                    w2d = c["w"].view(Nout, K).to(torch.bfloat16).contiguous()
                    runs = {}
                    for grid in (1, 2):
                        _C.gemm_tune("c1fwd_grid", grid)
                        b3, bd = copy.deepcopy(c["bn3"]), copy.deepcopy(c["bnd"])
                        a = [c["z3"], w2d, b3.weight.detach(), b3.bias.detach(), b3.running_mean, b3.running_var,
                             b3.num_batches_tracked, c["s3"].clone(), float(b3.momentum), float(b3.eps)]
                        if rbn:
                            a += [None, c["res"], bd.weight.detach(), bd.bias.detach(), bd.running_mean,
                                  bd.running_var, bd.num_batches_tracked, c["sd"].clone(), float(bd.momentum),
                                  float(bd.eps)]
                        else:
                            a += [c["res"]]
                        y, bits, z1, s1 = _C.conv1_fwd_fused(*a)[:4]
                        torch.cuda.synchronize()
                        runs[grid] = dict(y=y, bits=bits, z1=z1, s1=s1)
                    _report(f"conv1_fwd K={K} N={Nout} rbn={int(rbn)} M={N * hw * hw}", runs, "s1")
    finally:
        for k, v in old.items():
            _C.gemm_tune(k, v)


if __name__ == "__main__":
    main()
