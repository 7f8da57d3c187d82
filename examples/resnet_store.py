"""ResNet-50 trained from stored uint8 images, augmented on the GPU.

The images come from an ``ImageStore`` built from a ``.npy`` pair (uint8
``[M, H, W, 3]`` images, integer ``[M]`` labels) or, when none is given, from a
seeded random store. ``AugmentedBatches`` turns them into the stem's bf16
channels_last input with one kernel launch per batch (random resized crop,
flip, normalise). Fused kernels, bf16 autocast, fused SGD; a few steps, the
loss printed.

    python examples/resnet_store.py [--images x.npy --labels y.npy] [--device-store]

Started by the launcher (``RANK`` / ``WORLD_SIZE`` / ``LOCAL_RANK`` in the
environment) every rank trains on its ``DistributedSampler`` shard through
``DistributedDataParallel``.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import distributed_compute_pytorch_amd as dcp  # noqa: E402
from distributed_compute_pytorch_amd.models import resnet50  # noqa: E402
from distributed_compute_pytorch_amd.utils import AugmentedBatches, ImageStore, print0  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default=None, help=".npy, uint8 [M, H, W, 3] (opened as a memmap)")
    ap.add_argument("--labels", default=None, help=".npy, integer [M]")
    ap.add_argument("--device-store", action="store_true", help="keep the whole store in HBM")
    ap.add_argument("--batch", type=int, default=64, help="per rank")
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet_store needs a GPU")
    distributed = "WORLD_SIZE" in os.environ
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if distributed:
        dcp.distributed.init_process_group("rccl", device_id=local)
    torch.manual_seed(a.seed)

    if (a.images is None) != (a.labels is None):
        raise SystemExit("--images and --labels go together")
    if a.images is not None:
        import numpy as np

        images, labels = np.load(a.images, mmap_mode="r"), torch.from_numpy(np.load(a.labels))
    else:
        g = torch.Generator().manual_seed(a.seed)
        images = torch.randint(0, 256, (4 * a.batch, 256, 256, 3), dtype=torch.uint8, generator=g)
        labels = torch.randint(0, a.classes, (len(images),), generator=g)
    store = ImageStore(images, labels, device=dev if a.device_store else None)
    sampler = dcp.DistributedSampler(store, shuffle=True, seed=a.seed) if distributed else None
    batches = AugmentedBatches(store, sampler, batch_size=a.batch, size=a.size, device=dev)

    model = resnet50(num_classes=a.classes, fused_bn=True).to(dev).to(memory_format=torch.channels_last)
    if distributed:
        model = dcp.parallel.DistributedDataParallel(model, device_ids=[local], gradient_as_bucket_view=True)
    opt = dcp.optim.SGD(model.parameters(), lr=a.lr, momentum=0.9, weight_decay=1e-4)

    step, epoch = 0, 0
    while step < a.steps:
        batches.set_epoch(epoch)
        for x, y in batches:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = F.cross_entropy(model(x), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            step += 1
            print0(f"step {step} epoch {epoch} loss {loss.item():.4f}", rank=rank)
            if step == a.steps:
                break
        epoch += 1
    batches.close()
    if distributed:
        dcp.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
