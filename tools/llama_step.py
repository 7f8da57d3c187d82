"""Step time of the Llama model on one GPU, fused kernels against the plain
PyTorch variant (``fused=False``), timed the way bench.py times GPT-2: warm-up
steps, then K optimizer steps (each ``--accum`` micro-steps of forward +
backward under bf16 autocast) between two synchronizes.

    python tools/llama_step.py [--steps 10] [--warmup 5] [--batch 8] [--seq 1024] [--accum 4]
                               [--layers 12] [--only fused|plain] [--jsonl out.jsonl]

Prints one JSON line per variant: tokens/s, ms per step, final loss.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import distributed_compute_pytorch_amd as dcp  # noqa: E402
from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM  # noqa: E402


def run(fused, a, dev):
    torch.manual_seed(0)
    cfg = LlamaConfig(n_layer=a.layers, block_size=max(1024, a.seq))
    model = LlamaForCausalLM(cfg, fused=fused).to(dev)
    opt = dcp.optim.AdamW(model.parameters(), lr=3e-4, betas=(0.9, 0.95), weight_decay=0.1)
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, cfg.vocab, (4, a.batch, a.seq + 1), generator=g).to(dev)

    def step(i):
        opt.zero_grad(set_to_none=True)
        for k in range(a.accum):
            t = tok[(i * a.accum + k) % tok.shape[0]]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = model(t[:, :-1], t[:, 1:]) / a.accum
            loss.backward()
        opt.step()
        return loss

    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss = step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tokens = a.steps * a.accum * a.batch * a.seq
    return {"model": "llama_small", "fused": fused, "layers": a.layers, "batch": a.batch, "seq": a.seq,
            "accum": a.accum, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 2),
            "tokens_per_s": round(tokens / dt, 1), "loss": round(float(loss.detach()) * a.accum, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--only", choices=["fused", "plain"], default=None)
    ap.add_argument("--jsonl", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    for fused in (True, False):
        if a.only and (a.only == "fused") != fused:
            continue
        r = run(fused, a, dev)
        print(json.dumps(r), flush=True)
        if a.jsonl:
            with open(a.jsonl, "a") as f:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
