"""SwiGLU on the packed gate|up projection (csrc/kernels/swiglu.hip).

``swiglu(packed)`` with ``packed = [..., 2F]`` (the gate projection in the
first F columns, the up projection in the last F — one ``packed_linear`` of
the two weights) returns ``silu(gate) · up`` as ``[..., F]``. On a GPU with
bf16 input and ``F % 8 == 0`` one kernel runs each way: the forward reads the
packed input once and writes y; the backward reads dy and the saved packed
input and writes the packed gradient ``(d_gate | d_up)``, ``silu(gate)``
recomputed, never stored. Elsewhere (CPU, fp32, other F) it is
:func:`swiglu_reference`, the PyTorch formula that defines it.
"""
from __future__ import annotations

import torch
from torch.nn import functional as F_

from .._ext import C as _C


def swiglu_reference(packed: torch.Tensor) -> torch.Tensor:
    """The definition: fp32 arithmetic (fp64 for fp64 input), one rounding."""
    if packed.shape[-1] % 2:
        raise ValueError(f"swiglu: the last dim must be even (gate | up), got {packed.shape[-1]}")
    ct = torch.float64 if packed.dtype == torch.float64 else torch.float32
    gate, up = packed.to(ct).chunk(2, -1)
    return (F_.silu(gate) * up).to(packed.dtype)


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, packed):
        ctx.save_for_backward(packed)
        return _C.swiglu_fwd(packed)

    @staticmethod
    def backward(ctx, dy):
        (packed,) = ctx.saved_tensors
        dy = dy.contiguous()
        if dy.dtype != torch.bfloat16:
            dy = dy.to(torch.bfloat16)
        return _C.swiglu_bwd(dy, packed)


def swiglu(packed: torch.Tensor) -> torch.Tensor:
    if (packed.is_cuda and packed.dtype == torch.bfloat16 and packed.dim() >= 1 and packed.shape[-1] % 2 == 0
            and _C.swiglu_supported(packed.shape[-1] // 2)):
        return _SwiGLUFn.apply(packed.contiguous())
    return swiglu_reference(packed)
