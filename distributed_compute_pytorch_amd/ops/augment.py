"""On-device image augmentation (csrc/kernels/augment.hip).

``crop_resize_normalize(store, index, box, flip, size, mean, std)`` turns rows
of a uint8 ``[M, H, W, 3]`` image store into the stem's input: per sample the
crop ``box = (y0, x0, h, w)``, a bilinear resize to ``size x size``
(``align_corners=False``, not antialiased), an optional horizontal flip and
``(v / 255 - mean_c) / std_c``, written channels_last in bf16 (or fp32). On a
GPU store that is one kernel launch per batch, reading the store in place;
elsewhere it is :func:`crop_resize_normalize_reference`, the per-sample
PyTorch composition that defines it.

Boxes are integers, as torchvision's ``RandomResizedCrop.get_params`` draws
them: :func:`random_resized_crop_params` is that algorithm vectorised over the
batch on the host (reproducible under ``torch.manual_seed``), and
:func:`center_crop_params` gives the evaluation boxes. A box that sticks out
of the image is clamped into it and an index into ``[0, M)`` (kernel and
reference alike).
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch
from torch.nn import functional as F_

from .._ext import C as _C

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
ATTEMPTS = 10  # torchvision's RandomResizedCrop tries this many boxes


def affine(mean: Sequence[float], std: Sequence[float]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The per-channel fp32 (a, b) of ``v · a + b`` as the kernel receives
    them: a = 1 / (255 · std), b = −mean / std, formed in fp64, rounded once."""
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std must have 3 entries")
    a = torch.tensor([1.0 / (255.0 * float(s)) for s in std], dtype=torch.float64).float()
    b = torch.tensor([-float(m) / float(s) for m, s in zip(mean, std)], dtype=torch.float64).float()
    return a, b


def clamp_box(box, H: int, W: int):
    """(y0, x0, h, w) clamped as the kernel clamps it: the origin into the
    image, then the extent into what is left of it (at least one pixel)."""
    y0, x0, h, w = (int(v) for v in box)
    y0, x0 = min(max(y0, 0), H - 1), min(max(x0, 0), W - 1)
    return y0, x0, min(max(h, 1), H - y0), min(max(w, 1), W - x0)


def crop_resize_normalize_reference(store, index, box, flip, size, mean, std, dtype=torch.bfloat16):
    """The definition, sample by sample: crop, ``F.interpolate`` (bilinear,
    ``align_corners=False``, ``antialias=False``) in fp32, flip, ``v·a + b``,
    one rounding to ``dtype``; stacked and laid out channels_last."""
    M, H, W = store.shape[0], store.shape[1], store.shape[2]
    a, b = (t.to(store.device).view(3, 1, 1) for t in affine(mean, std))
    index, box, flip = index.tolist(), box.tolist(), flip.tolist()
    out = torch.empty((len(index), 3, size, size), dtype=dtype, device=store.device,
                      memory_format=torch.channels_last)
    for i, (row, bx, fl) in enumerate(zip(index, box, flip)):
        y0, x0, h, w = clamp_box(bx, H, W)
        crop = store[min(max(row, 0), M - 1), y0:y0 + h, x0:x0 + w].permute(2, 0, 1).float().unsqueeze(0)
        r = F_.interpolate(crop, size=(size, size), mode="bilinear", align_corners=False, antialias=False)[0]
        if fl:
            r = r.flip(-1)
        out[i] = (r * a + b).to(dtype)
    return out


def crop_resize_normalize(store: torch.Tensor, index: torch.Tensor, box: torch.Tensor, flip: torch.Tensor, size: int,
                          mean: Sequence[float] = IMAGENET_MEAN, std: Sequence[float] = IMAGENET_STD,
                          dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """``[N, 3, size, size]`` channels_last from rows ``index`` of ``store``."""
    if store.dim() != 4 or store.shape[3] != 3 or store.dtype != torch.uint8:
        raise ValueError(f"store must be uint8 [M, H, W, 3], got {store.dtype} {tuple(store.shape)}")
    if box.shape != (index.shape[0], 4) or flip.shape != index.shape:
        raise ValueError("index [N], box [N, 4] and flip [N] must agree on N")
    if store.is_cuda:
        dev = store.device
        return _C.crop_resize_norm(store.contiguous(), index.to(dev, torch.int64).contiguous(),
                                   box.to(dev, torch.int32).contiguous(), flip.to(dev, torch.uint8).contiguous(),
                                   int(size), [float(m) for m in mean], [float(s) for s in std], dtype)
    return crop_resize_normalize_reference(store, index, box, flip, int(size), mean, std, dtype)


def random_resized_crop_params(n: int, H: int, W: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0),
                               p_flip: float = 0.5, generator: Optional[torch.Generator] = None,
                               uniforms=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """torchvision's ``RandomResizedCrop.get_params`` for ``n`` images of
    ``H x W`` at once, plus the flip coin: ``(box int32 [n, 4], flip uint8 [n])``.

    Per attempt (10 of them): the area uniform in ``scale · H · W``, the aspect
    ratio log-uniform in ``ratio``, ``w = round(sqrt(area · r))``, ``h =
    round(sqrt(area / r))``; the first attempt with ``0 < w <= W`` and ``0 < h
    <= H`` wins and its top-left corner is uniform over the valid integers;
    with none, the central crop with the image's ratio clamped into ``ratio``.

    ``uniforms = (u, uf)`` injects the random numbers: ``u`` ``[n, 10, 4]`` in
    [0, 1) (area, log-ratio, top, left per attempt) and ``uf`` ``[n]`` (flip
    when ``uf < p_flip``). Otherwise they are drawn from ``generator`` (the
    global CPU generator when None) on the host."""
    if uniforms is None:
        u = torch.rand((n, ATTEMPTS, 4), dtype=torch.float64, generator=generator)
        uf = torch.rand((n,), dtype=torch.float64, generator=generator)
    else:
        u, uf = (torch.as_tensor(t, dtype=torch.float64) for t in uniforms)
        if u.shape != (n, ATTEMPTS, 4) or uf.shape != (n,):
            raise ValueError(f"uniforms must be ([{n}, {ATTEMPTS}, 4], [{n}])")
    area = float(H * W) * (scale[0] + (scale[1] - scale[0]) * u[..., 0])
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    r = torch.exp(lo + (hi - lo) * u[..., 1])
    w = torch.round(torch.sqrt(area * r)).to(torch.int64)  # half to even, as Python's round
    h = torch.round(torch.sqrt(area / r)).to(torch.int64)
    ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    any_ok = ok.any(dim=1)
    first = torch.argmax(ok.to(torch.int8), dim=1, keepdim=True)  # first accepted attempt (0 if none)
    w, h = w.gather(1, first)[:, 0], h.gather(1, first)[:, 0]
    ut, ul = u[..., 2].gather(1, first)[:, 0], u[..., 3].gather(1, first)[:, 0]
    # the central fallback: the whole image, cut to the nearest allowed ratio
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        fw, fh = W, int(round(W / min(ratio)))
    elif in_ratio > max(ratio):
        fh, fw = H, int(round(H * max(ratio)))
    else:
        fw, fh = W, H
    w = torch.where(any_ok, w, torch.full_like(w, fw))
    h = torch.where(any_ok, h, torch.full_like(h, fh))
    # randint(0, H − h + 1) as floor(u · (H − h + 1)); the min guards u · k == k after rounding
    top = torch.minimum(torch.floor(ut * (H - h + 1).double()).to(torch.int64), H - h)
    left = torch.minimum(torch.floor(ul * (W - w + 1).double()).to(torch.int64), W - w)
    top = torch.where(any_ok, top, (H - h) // 2)
    left = torch.where(any_ok, left, (W - w) // 2)
    box = torch.stack([top, left, h, w], dim=1).to(torch.int32)
    return box, (uf < p_flip).to(torch.uint8)


def center_crop_params(n: int, H: int, W: int, crop_frac: float = 0.875) -> Tuple[torch.Tensor, torch.Tensor]:
    """Evaluation boxes: the central square of side ``round(crop_frac ·
    min(H, W))`` (resize-then-centre-crop at the usual 0.875), no flip."""
    c = max(1, min(H, W, int(round(crop_frac * min(H, W)))))
    box = torch.tensor([[(H - c) // 2, (W - c) // 2, c, c]], dtype=torch.int32).repeat(n, 1)
    return box, torch.zeros(n, dtype=torch.uint8)
