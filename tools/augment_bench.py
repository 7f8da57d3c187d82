"""Measure the on-device image augmentation path on one GPU and write
profiles/augment_bench.json:

* crop_resize_norm_kernel on [B, 256, 256, 3] -> 224, bf16: µs per launch
  (device events around a run of launches, several runs) and the effective
  TB/s against its byte model (the whole batch read once + the output written);
* the stock composition (per-sample crop, F.interpolate, flip, normalise) on
  the same batch, for the ratio;
* the pinned -> device copy of one [B, H, W, 3] batch;
* AugmentedBatches alone, images/s, host and device store;
* the ResNet-50 training step (bench.py's eager configuration: DDP at world
  size 1, bf16 autocast, fused SGD) fed by SyntheticBatches, by a device store
  and by a host store — one process, the variants alternated block by block,
  --blocks timed blocks each, every block's ms/step on record together with
  the loader's own host timers (row gather, consumer blocked on the queue).

    python tools/augment_bench.py [--batch 1024] [--blocks 3] [--steps 8] [--skip-step]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _LongSampler:
    """``n`` indices drawn with replacement: one long epoch, so the loader's
    prefetch never restarts inside a timed block."""

    def __init__(self, M, n, seed=0):
        self.idx = torch.randint(0, M, (n,), generator=torch.Generator().manual_seed(seed)).tolist()

    def __iter__(self):
        return iter(self.idx)

    def __len__(self):
        return len(self.idx)


def _events_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _spread(xs):
    return {"runs": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--store", type=int, default=4096, help="images in the store")
    ap.add_argument("--hw", type=int, default=256, help="stored image side")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks per variant (>= 3)")
    ap.add_argument("--steps", type=int, default=8, help="steps per timed block")
    ap.add_argument("--warmup", type=int, default=6, help="untimed ResNet steps before the first block")
    ap.add_argument("--skip-step", action="store_true", help="kernel and loader only, no ResNet-50 step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs a GPU: nothing here can be measured without one")

    import distributed_compute_pytorch_amd as dcp
    from distributed_compute_pytorch_amd import ops, workloads
    from distributed_compute_pytorch_amd.utils import AugmentedBatches, ImageStore

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, M, H, S = a.batch, a.store, a.hw, a.size
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (M, H, H, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 1000, (M,), generator=g)
    dimages = images.to(dev)
    res = {"shape": {"batch": B, "store": [M, H, H, 3], "size": S, "dtype": "bf16"},
           "device": torch.cuda.get_device_name(0)}

    # ---- the kernel alone ------------------------------------------------
    index = torch.randint(0, M, (B,), generator=g).to(dev)
    box, flip = ops.random_resized_crop_params(B, H, H, generator=g)
    dbox, dflip = box.to(dev), flip.to(dev)
    kern = lambda: ops.crop_resize_normalize(dimages, index, dbox, dflip, S)  # noqa: E731
    for _ in range(5):
        kern()
    torch.cuda.synchronize()
    us = [_events_ms(kern, 50) * 1e3 for _ in range(5)]
    nbytes = B * H * H * 3 + B * S * S * 3 * 2
    res["kernel_us"] = _spread(us)
    res["kernel_byte_model_MB"] = round(nbytes / 1e6, 1)
    res["kernel_effective_TBps"] = round(nbytes / (statistics.median(us) * 1e-6) / 1e12, 3)
    whole = torch.tensor([[0, 0, H, H]], dtype=torch.int32).repeat(B, 1).to(dev)  # every source byte is read
    kern_whole = lambda: ops.crop_resize_normalize(dimages, index, whole, dflip, S)  # noqa: E731
    kern_whole()
    us_w = [_events_ms(kern_whole, 50) * 1e3 for _ in range(5)]
    res["kernel_whole_image_us"] = _spread(us_w)
    res["kernel_whole_image_TBps"] = round(nbytes / (statistics.median(us_w) * 1e-6) / 1e12, 3)
    print(f"[augment_bench] kernel {res['kernel_us']} us, {res['kernel_effective_TBps']} TB/s of the byte model",
          flush=True)

    # ---- the stock composition on the same batch -----------------------
    stock = lambda: ops.crop_resize_normalize_reference(dimages, index, dbox, dflip, S, ops.augment.IMAGENET_MEAN,  # noqa: E731
                                                        ops.augment.IMAGENET_STD)
    stock()
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        stock()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    res["stock_composition_ms"] = _spread(ms)
    res["stock_over_kernel"] = round(statistics.median(ms) * 1e3 / statistics.median(us), 1)
    print(f"[augment_bench] stock composition {res['stock_composition_ms']} ms", flush=True)

    # ---- the host -> device copy of one batch ----------------------------
    pinned = torch.empty((B, H, H, 3), dtype=torch.uint8).pin_memory()
    dst = torch.empty((B, H, H, 3), dtype=torch.uint8, device=dev)
    dst.copy_(pinned, non_blocking=True)
    cp = [_events_ms(lambda: dst.copy_(pinned, non_blocking=True), 5) for _ in range(3)]
    res["h2d_batch_copy_ms"] = _spread(cp)
    res["h2d_GBps"] = round(B * H * H * 3 / (statistics.median(cp) * 1e-3) / 1e9, 1)
    del pinned, dst

    # ---- the loader alone ------------------------------------------------
    nb = 10
    for name, store in (("device", ImageStore(dimages, labels, device=dev)), ("host", ImageStore(images, labels))):
        rates, stats = [], []
        for blk in range(a.blocks + 1):  # block 0 warms the pinned buffers up
            it = AugmentedBatches(store, _LongSampler(M, nb * B, seed=blk), batch_size=B, size=S, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for x, y in it:
                pass
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if blk:
                rates.append(nb * B / dt)
                stats.append({k: round(v / nb * 1e3, 2) for k, v in it.stats.items() if k != "batches"})
        res[f"loader_{name}_store_images_per_s"] = _spread(rates)
        res[f"loader_{name}_store_ms_per_batch"] = stats  # gather_s / wait_s per batch, in ms
        print(f"[augment_bench] loader alone, {name} store: {res[f'loader_{name}_store_images_per_s']} img/s",
              flush=True)

    # ---- the ResNet-50 step ------------------------------------------------
    if not a.skip_step:
        from distributed_compute_pytorch_amd.distributed.launch import free_port

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1")
        dcp.distributed.init_process_group("rccl", device_id=0)
        wl = workloads.build("resnet50", dev, batch=B)
        ddp = dcp.parallel.DistributedDataParallel(wl.model, device_ids=[0], gradient_as_bucket_view=True,
                                                   **dcp.parallel.XGMI_BUCKETS)
        opt = wl.make_optimizer(ddp.parameters())
        step = workloads.make_step(wl, ddp, opt)
        total = (a.blocks + 1) * (a.steps + 2) * B
        loaders = {"device": AugmentedBatches(ImageStore(dimages, labels, device=dev), _LongSampler(M, total, 1),
                                              batch_size=B, size=S, device=dev),
                   "host": AugmentedBatches(ImageStore(images, labels), _LongSampler(M, total, 2), batch_size=B,
                                            size=S, device=dev)}
        feeds = {"synthetic": wl.data, "device": iter(loaders["device"]), "host": iter(loaders["host"])}
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        out = {k: [] for k in feeds}
        timers = {k: [] for k in loaders}
        for blk in range(a.blocks):
            for name, feed in feeds.items():  # alternated: one block of each per round
                wl.data = feed
                before = dict(loaders[name].stats) if name in loaders else None
                for _ in range(2):
                    loss = step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    loss = step()
                torch.cuda.synchronize()
                out[name].append((time.perf_counter() - t0) / a.steps * 1e3)
                if before is not None:
                    st = loaders[name].stats
                    n = st["batches"] - before["batches"]
                    timers[name].append({k: round((st[k] - before[k]) / n * 1e3, 2) for k in ("gather_s", "wait_s")})
                print(f"[augment_bench] block {blk} {name}: {out[name][-1]:.2f} ms/step loss={float(loss.detach()):.3f}",
                      flush=True)
        res["resnet50_step_ms"] = {k: _spread(v) for k, v in out.items()}
        res["resnet50_images_per_s"] = {k: round(B / statistics.median(v) * 1e3, 1) for k, v in out.items()}
        res["resnet50_vs_synthetic"] = {k: round(statistics.median(v) / statistics.median(out["synthetic"]), 4)
                                        for k, v in out.items()}
        res["resnet50_loader_ms_per_batch"] = timers
        for it in loaders.values():
            it.close()
        dcp.distributed.destroy_process_group()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
