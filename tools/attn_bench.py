"""Attention fwd / fwd+bwd at the BERT-base (B32 T512 H12, dropout 0.1) and
GPT-2-small (B8 T1024 H12 causal, dropout 0.1) shapes: our MFMA flash
attention vs torch scaled_dot_product_attention (aotriton on ROCm). Two more
cases run the BERT shape with a key-padding mask: ``bert-pad`` (per-sequence
lengths drawn once from a seeded generator, uniform in [128, 512], right-padded)
and ``bert-pad-full`` (an all-True mask: the price of carrying the mask);
scaled_dot_product_attention gets the same boolean mask as [B, 1, 1, T].
``llama-d128`` is the head-dim-128 kernel family at B8 T1024, 12 heads of 128,
causal, no dropout (profiles/attn_d128_bench.jsonl: ``--cases llama-d128
--iters 50 --repeat 5 --out profiles/attn_d128_bench.jsonl``).
``mistral-swa`` is the sliding-window variant of that family at B1 T8192, 8
heads of 128: ``window=1024`` and ``window=4096`` against the unwindowed causal
kernels at the same shape (no SDPA column: the yardstick is our own causal
path), the three alternating; ``*_vs_causal`` is the time ratio and
``*_blocks_vs_causal`` the ratio of visited 64-key blocks it is to be read
against (profiles/attn_window_bench.jsonl).

    python tools/attn_bench.py [--iters 10] [--graph 1] [--repeat 1] [--out FILE]

--repeat N takes every timing N times, ours and SDPA alternating, and reports
the median plus ``*_spread_us`` (max - min): the run-to-run spread a difference
has to exceed.

--graph 1 (default) times replays of a captured HIP graph of each call, so
the numbers are GPU time (the eager loop's autograd / launch overhead per
fwd+bwd, ~40-50 µs, exceeds the BERT-shape kernels' idle slack); --graph 0
times the eager calls.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_compute_pytorch_amd.ops.attention import flash_attn, pack_key_mask  # noqa: E402


GRAPH = True


def timeit(fn, iters):
    # three warm-up calls: the process's first two backward passes carry the
    # autograd engine's one-time start-up (0.7 s + 70 ms, tools/attn_diag.py)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    run = fn
    if GRAPH:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        run = g.replay
        run()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cases", nargs="*", default=None,
                    help="subset of bert gpt2 bert-nodrop gpt2-nodrop bert-pad bert-pad-full llama-d128 mistral-swa")
    ap.add_argument("--graph", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    global GRAPH
    GRAPH = bool(a.graph)
    dev = torch.device("cuda", 0)

    def rounds(r, key, fns):
        """the variants of ``fns`` timed a.repeat times, alternating; median (+ spread)"""
        runs = {who: [] for who in fns}
        for _ in range(a.repeat):
            for who, fn in fns.items():
                runs[who].append(timeit(fn, a.iters))
        for who, ts in runs.items():
            r[f"{who}_{key}_us"] = sorted(ts)[len(ts) // 2]
            if a.repeat > 1:
                r[f"{who}_{key}_spread_us"] = max(ts) - min(ts)

    def pair(r, key, ours, sdpa):
        rounds(r, key, {"ours": ours, "sdpa": sdpa})

    def emit(r):
        line = json.dumps({kk: (round(vv, 3 if kk.endswith("_vs_causal") else 1) if isinstance(vv, float) else vv)
                           for kk, vv in r.items()})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    if not a.cases or "mistral-swa" in a.cases:
        B, T, H, D = 1, 8192, 8, 128
        q, k, v, do = (torch.randn(B, T, H * D, device=dev, dtype=torch.bfloat16) for _ in range(4))
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        kws = {"w1024": {"window": 1024}, "w4096": {"window": 4096}, "causal": {}}
        r = {"case": "mistral-swa", "graph": GRAPH, "iters": a.iters, "repeat": a.repeat}
        rounds(r, "fwd", {n: (lambda kw=kw: flash_attn(q, k, v, H, True, **kw)) for n, kw in kws.items()})
        rounds(r, "fwdbwd", {n: (lambda kw=kw: torch.autograd.grad(flash_attn(qa, ka, va, H, True, **kw),
                                                                   (qa, ka, va), do)) for n, kw in kws.items()})
        # 64-key blocks a 128-query tile stages: min(T/64, 2·tile + 2) − it_lo (attention_d128.hip)
        blocks = lambda W: sum(2 * t + 2 - max(0, 128 * t - W + 1) // 64 for t in range(T // 128))
        for n, W in (("w1024", 1024), ("w4096", 4096)):
            r[f"{n}_blocks_vs_causal"] = blocks(W) / blocks(T)
            for key in ("fwd", "fwdbwd"):
                r[f"{n}_{key}_vs_causal"] = r[f"{n}_{key}_us"] / r[f"causal_{key}_us"]
        emit(r)

    for name, B, T, H, causal, p, pad, D in [("bert", 32, 512, 12, False, 0.1, None, 64),
                                             ("gpt2", 8, 1024, 12, True, 0.1, None, 64),
                                             ("bert-nodrop", 32, 512, 12, False, 0.0, None, 64),
                                             ("gpt2-nodrop", 8, 1024, 12, True, 0.0, None, 64),
                                             ("bert-pad", 32, 512, 12, False, 0.1, "lengths", 64),
                                             ("bert-pad-full", 32, 512, 12, False, 0.1, "full", 64),
                                             ("llama-d128", 8, 1024, 12, True, 0.0, None, 128)]:
        if a.cases and name not in a.cases:
            continue
        C = H * D
        km = am = None  # the packed key mask (packed once, as a model does) / SDPA's boolean attn_mask
        if pad is not None:
            lens = torch.full((B,), T)
            if pad == "lengths":
                lens = torch.randint(128, T + 1, (B,), generator=torch.Generator().manual_seed(0))
            mask = (torch.arange(T)[None, :] < lens[:, None]).to(dev)
            km, am = pack_key_mask(mask), mask[:, None, None, :]
        q, k, v, do = (torch.randn(B, T, C, device=dev, dtype=torch.bfloat16) for _ in range(4))
        qs, ks, vs = (t.view(B, T, H, D).transpose(1, 2) for t in (q, k, v))
        fl = 4.0 * B * H * T * T * D * (0.5 if causal else 1.0)
        r = {"case": name, "graph": GRAPH, "iters": a.iters, "repeat": a.repeat}
        if pad is not None:
            r["mean_len"] = float(lens.float().mean())
        mkw = {} if km is None else {"key_mask": km}    # (no mask: the call of the unmasked cases, unchanged)
        skw = {} if am is None else {"attn_mask": am}
        pair(r, "fwd", lambda: flash_attn(q, k, v, H, causal, p, **mkw),
             lambda: F.scaled_dot_product_attention(qs, ks, vs, dropout_p=p, is_causal=causal, **skw))
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))

        # torch.autograd.grad: the gradients come back as new tensors, as in a
        # training step (where they feed the projection's backward) — a
        # .backward() here would add three [B, T, C] .grad accumulations
        # (~45 µs at the BERT shape) to every fwd+bwd
        def ours_fb():
            torch.autograd.grad(flash_attn(qa, ka, va, H, causal, p, **mkw), (qa, ka, va), do)

        qsa, ksa, vsa = (t.clone().requires_grad_(True) for t in (qs, ks, vs))
        dos = do.view(B, T, H, D).transpose(1, 2)

        def sdpa_fb():
            torch.autograd.grad(
                F.scaled_dot_product_attention(qsa, ksa, vsa, dropout_p=p, is_causal=causal, **skw),
                (qsa, ksa, vsa), dos)

        pair(r, "fwdbwd", ours_fb, sdpa_fb)
        r["ours_fwd_TFps"] = fl / (r["ours_fwd_us"] * 1e-6) / 1e12
        r["ours_fwdbwd_TFps"] = 3.5 * fl / (r["ours_fwdbwd_us"] * 1e-6) / 1e12
        emit(r)


if __name__ == "__main__":
    main()
