"""Real-image input path: a uint8 image store and batches augmented on the GPU.

* :class:`ImageStore` — decoded RGB images as one uint8 ``[M, H, W, 3]`` array
  (a tensor, a numpy array or a memmap) with int64 labels. With ``device=`` the
  images live in HBM (a rank's shard, or a whole small set) and the
  augmentation kernel indexes them in place; without, they stay on the host.
* :class:`AugmentedBatches` — an iterator of ``(x, y)`` on the GPU: ``x`` bf16
  channels_last ``[B, 3, S, S]`` from ``ops.crop_resize_normalize`` (random
  resized crop + flip when ``train``, the central crop otherwise), ``y`` int64
  ``[B]``. One background thread (alive while an epoch is in flight) prepares
  batch k+1 while step k runs:

  - host store: it gathers the batch's rows into one of two pinned uint8
    buffers, then enqueues the ``[B, H, W, 3]`` copy, the parameter copy and
    the kernel on a side stream;
  - device store: only the packed index / label / box / flip copy and the
    kernel are enqueued.

  An event hands the finished batch to the consumer's stream, and what is
  handed over is marked with ``record_stream``. The crop parameters are drawn
  on the host in the consumer's thread, in batch order, so the stream of
  batches is reproducible under ``torch.manual_seed`` (or ``generator=``).
  No worker processes: nothing depends on the core count. The iterator sits
  outside a captured step; its batches are copied into the step's static
  inputs like any others.
"""
from __future__ import annotations

import queue
import threading
import time
from typing import Optional, Sequence

import torch

from ..ops.augment import (IMAGENET_MEAN, IMAGENET_STD, center_crop_params, crop_resize_normalize,
                           random_resized_crop_params)


class ImageStore:
    """uint8 ``[M, H, W, 3]`` images + int64 ``[M]`` labels."""

    def __init__(self, images, labels, device=None):
        self._np = None
        if not isinstance(images, torch.Tensor):
            import numpy as np

            if not isinstance(images, np.ndarray) or images.dtype != np.uint8:
                raise TypeError("images must be a uint8 tensor or numpy array")
            if device is None:
                self._np = images  # memmaps stay on disk / in the page cache; rows are read per batch
            images = None if device is None else torch.from_numpy(np.ascontiguousarray(images))
        shape = tuple(self._np.shape) if images is None else tuple(images.shape)
        if len(shape) != 4 or shape[3] != 3 or (images is not None and images.dtype != torch.uint8):
            raise ValueError(f"images must be uint8 [M, H, W, 3], got {shape}")
        labels = torch.as_tensor(labels).to(torch.int64).cpu().contiguous()
        if labels.shape != (shape[0],):
            raise ValueError(f"labels must be [{shape[0]}], got {tuple(labels.shape)}")
        self.shape = shape
        self.labels = labels  # on the host: a batch's labels travel with its parameters
        self.device = torch.device("cpu") if device is None else torch.device(device)
        self.images = None if images is None else images.to(self.device).contiguous()

    def __len__(self) -> int:
        return self.shape[0]

    @property
    def on_device(self) -> bool:
        return self.device.type == "cuda"

    def gather(self, idx: torch.Tensor, out: torch.Tensor) -> None:
        """rows ``idx`` (int64, host) of a host store into ``out`` ``[n, H, W, 3]``."""
        if self._np is not None:
            import numpy as np

            np.take(self._np, idx.numpy(), axis=0, out=out.numpy())
        else:
            torch.index_select(self.images, 0, idx, out=out)


class AugmentedBatches:
    def __init__(self, store: ImageStore, sampler=None, batch_size: int = 256, size: int = 224, train: bool = True,
                 mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD,
                 generator: Optional[torch.Generator] = None, drop_last: bool = True, device=None,
                 dtype: torch.dtype = torch.bfloat16):
        self.store, self.sampler = store, sampler
        self.batch_size, self.size, self.train = int(batch_size), int(size), train
        self.mean, self.std = tuple(mean), tuple(std)
        self.generator, self.drop_last, self.dtype = generator, drop_last, dtype
        if device is None:
            device = store.device if store.on_device else (
                torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu")
        self.device = torch.device(device)
        if store.on_device and self.device != store.device:
            raise ValueError(f"the store is on {store.device}, the batches were asked for on {self.device}")
        self.stats = {"batches": 0, "gather_s": 0.0, "wait_s": 0.0}  # host clocks: row gather, consumer blocked
        self._jobs: Optional[queue.Queue] = None
        self._done: queue.Queue = queue.Queue()
        self._thread: Optional[threading.Thread] = None
        self._pinned = [None, None]  # per slot: (packed parameters, image rows), allocated on first use
        self._copied = [None, None]  # per slot: event behind the slot's last host-to-device copies
        self._side = None  # the stream the copies and the kernel run on
        self._batches = []
        self._next = self._issued = 0

    # ------------------------------------------------------------ epochs ---
    def set_epoch(self, epoch: int) -> None:
        if hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def __len__(self) -> int:
        n = len(self.sampler) if self.sampler is not None else len(self.store)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        self._drain()
        idx = torch.as_tensor(list(self.sampler) if self.sampler is not None else range(len(self.store)),
                              dtype=torch.int64)
        B = self.batch_size
        self._batches = [idx[i:i + B] for i in range(0, len(idx), B)]
        if self.drop_last and self._batches and len(self._batches[-1]) < B:
            self._batches.pop()
        self._next = self._issued = 0
        self._issue()
        return self

    def __next__(self):
        if self._next >= len(self._batches):
            raise StopIteration
        if self.device.type != "cuda":
            batch = self._pending
        else:
            t0 = time.perf_counter()
            batch = self._done.get()
            self.stats["wait_s"] += time.perf_counter() - t0
            if isinstance(batch, BaseException):
                self._next = len(self._batches)
                raise batch
            x, y, packed, ready = batch
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ready)
            for t in (x, packed):  # y is a view of packed
                t.record_stream(cur)
            batch = (x, y)
        self._next += 1
        self.stats["batches"] += 1
        self._issue()  # batch k+1 is prepared while the caller runs step k
        return batch

    # ----------------------------------------------------------- workers ---
    def _params(self, n: int):
        _, H, W, _ = self.store.shape
        if self.train:
            return random_resized_crop_params(n, H, W, generator=self.generator)
        return center_crop_params(n, H, W)

    def _issue(self) -> None:
        k = self._issued
        if k >= len(self._batches):
            return
        self._issued += 1
        idx = self._batches[k]
        box, flip = self._params(len(idx))  # drawn here, in batch order, in the consumer's thread
        if self.device.type != "cuda":
            x = crop_resize_normalize(self.store.images if self.store._np is None else
                                      torch.from_numpy(self.store._np[idx.numpy()]),
                                      idx if self.store._np is None else torch.arange(len(idx)), box, flip,
                                      self.size, self.mean, self.std, self.dtype)
            self._pending = (x, self.store.labels[idx])
            return
        if self._thread is None:
            self._jobs = queue.Queue()
            self._thread = threading.Thread(target=self._work, args=(self._jobs,), name="dcp-augment", daemon=True)
            self._thread.start()
        self._jobs.put((k % 2, idx, box, flip))
        if self._issued == len(self._batches):  # the epoch's last job: the thread ends behind it
            self._jobs.put(None)
            self._thread = self._jobs = None

    def _work(self, jobs: queue.Queue) -> None:
        torch.cuda.set_device(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        side = self._side
        while True:
            job = jobs.get()
            if job is None:
                return
            try:
                self._done.put(self._prepare(side, *job))
            except BaseException as e:  # handed to the consumer, which raises it
                self._done.put(e)

    def _prepare(self, side, slot: int, idx: torch.Tensor, box: torch.Tensor, flip: torch.Tensor):
        n, B = len(idx), self.batch_size
        _, H, W, _ = self.store.shape
        host = not self.store.on_device
        if self._pinned[slot] is None:
            self._pinned[slot] = (torch.empty(33 * B, dtype=torch.uint8).pin_memory(),
                                  torch.empty((B, H, W, 3), dtype=torch.uint8).pin_memory() if host else None)
        if self._copied[slot] is not None:
            self._copied[slot].synchronize()  # the slot's previous copies have left the pinned buffers
        packed, rows = self._pinned[slot]
        # one packed parameter copy: index int64 | labels int64 | box int32 x 4 | flip uint8
        packed[0:8 * n].view(torch.int64).copy_(torch.arange(n) if host else idx)
        packed[8 * n:16 * n].view(torch.int64).copy_(self.store.labels[idx])
        packed[16 * n:32 * n].view(torch.int32).copy_(box.reshape(-1))
        packed[32 * n:33 * n].copy_(flip)
        if host:
            t0 = time.perf_counter()
            self.store.gather(idx, rows[:n])
            self.stats["gather_s"] += time.perf_counter() - t0
        with torch.cuda.stream(side):
            dpacked = packed[:33 * n].to(self.device, non_blocking=True)
            images = rows[:n].to(self.device, non_blocking=True) if host else self.store.images
            self._copied[slot] = torch.cuda.Event()
            self._copied[slot].record(side)
            x = crop_resize_normalize(images, dpacked[0:8 * n].view(torch.int64),
                                      dpacked[16 * n:32 * n].view(torch.int32).view(n, 4), dpacked[32 * n:33 * n],
                                      self.size, self.mean, self.std, self.dtype)
            ready = torch.cuda.Event()
            ready.record(side)
        return x, dpacked[8 * n:16 * n].view(torch.int64), dpacked, ready

    def _drain(self) -> None:
        """Collect what an abandoned epoch left in flight."""
        while self._next < self._issued and self.device.type == "cuda":
            self._done.get()
            self._next += 1

    def close(self) -> None:
        """Stop the background thread of an epoch that was not run to its end
        (a finished epoch's thread has ended by itself)."""
        self._drain()
        if self._thread is not None:
            self._jobs.put(None)
            self._thread.join()
            self._thread = self._jobs = None
        self._batches, self._next, self._issued = [], 0, 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
