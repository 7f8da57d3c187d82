"""Rotary position embedding on the packed qkv projection (csrc/kernels/rope.hip).

``apply_rope_qkv(qkv, heads, table)`` rotates the q and k thirds of a packed
``[B, T, 3·heads·64]`` projection — the tensor ``flash_attn_qkv`` reads — and
leaves v alone. Head dim 64, rotate-half pairing ``(i, i + 32)``::

    y[i]      = x[i]·cos θ(t, i) − x[i + 32]·sin θ(t, i)
    y[i + 32] = x[i + 32]·cos θ(t, i) + x[i]·sin θ(t, i)      θ(t, i) = t · base^(−i / 32)

in fp32, rounded once. ``table = rope_table(T_max, base, device)`` holds
cos / sin as fp32 ``[T_max, 2, 32]`` (``table[t, 0]`` = cos, ``table[t, 1]`` =
sin), cached per (T_max, base, device); row ``t`` serves position ``t``.

The backward is the rotation by −θ of the incoming packed gradient: it needs
the table only, the forward saves nothing.

``inplace=True`` rotates ``qkv`` itself (``mark_dirty``): only the q and k
thirds move, 2/3 of the bytes each way. It is meant for the output of the
projection GEMM, whose backward does not read its own output; a leaf that
requires grad, or a view, is rotated out of place regardless. The backward
always writes a new tensor: the incoming gradient belongs to autograd (other
consumers, hooks, ``retain_grad``) and is not modified.

On the CPU, for other dtypes than bf16 and for fp32-only callers the op is
:func:`rope_qkv_reference`, the PyTorch formula that defines it.
"""
from __future__ import annotations

import torch

from .._ext import C as _C

_TABLES: dict = {}


def rope_table(T: int, base: float = 10000.0, device=None) -> torch.Tensor:
    """fp32 [T, 2, 32]: cos (index 0) and sin (index 1) of t · base^(−i/32),
    computed in fp64 and rounded once. Cached: build it outside graph capture
    (the model does, at its first forward)."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    key = (int(T), float(base), dev)
    t = _TABLES.get(key)
    if t is None:
        inv = torch.tensor(float(base), dtype=torch.float64) ** (-torch.arange(32, dtype=torch.float64) / 32.0)
        ang = torch.arange(int(T), dtype=torch.float64)[:, None] * inv[None, :]
        t = _TABLES[key] = torch.stack([ang.cos(), ang.sin()], 1).to(torch.float32).contiguous().to(dev)
    return t


def rope_qkv_reference(qkv: torch.Tensor, heads: int, table: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    """The definition, out of place, differentiable through autograd."""
    B, T, C3 = qkv.shape
    if C3 != 3 * heads * 64:
        raise ValueError(f"apply_rope_qkv: last dim must be 3*heads*64 = {3 * heads * 64}, got {C3}")
    if T > table.shape[0]:
        raise ValueError(f"apply_rope_qkv: sequence length {T} exceeds the table's {table.shape[0]} rows")
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    cos = table[:T, 0].to(device=qkv.device, dtype=ct)[None, :, None, :]
    sin = table[:T, 1].to(device=qkv.device, dtype=ct)[None, :, None, :]
    if inverse:
        sin = -sin
    qk = qkv[..., :2 * heads * 64].to(ct).reshape(B, T, 2 * heads, 64)
    a, b = qk[..., :32], qk[..., 32:]
    rot = torch.cat([a * cos - b * sin, b * cos + a * sin], -1).reshape(B, T, 2 * heads * 64)
    return torch.cat([rot.to(qkv.dtype), qkv[..., 2 * heads * 64:]], -1)


class _RopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, table, inplace):
        ctx.heads = heads
        ctx.save_for_backward(table)
        out = _C.rope_qkv(qkv, heads, table, False, inplace)
        if inplace:
            ctx.mark_dirty(qkv)
            return qkv
        return out

    @staticmethod
    def backward(ctx, g):
        (table,) = ctx.saved_tensors
        g = g.contiguous()
        if g.dtype != torch.bfloat16:
            g = g.to(torch.bfloat16)
        return _C.rope_qkv(g, ctx.heads, table, True, False), None, None, None


def apply_rope_qkv(qkv: torch.Tensor, heads: int, table: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    if (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3 and qkv.shape[2] == 3 * heads * 64
            and table.is_cuda and table.dtype == torch.float32 and tuple(table.shape[1:]) == (2, 32)
            and table.is_contiguous()):
        if qkv.shape[1] > table.shape[0]:
            raise ValueError(f"apply_rope_qkv: sequence length {qkv.shape[1]} exceeds the table's "
                             f"{table.shape[0]} rows")
        ip = bool(inplace) and qkv.is_contiguous() and not qkv._is_view() and not (qkv.is_leaf and qkv.requires_grad)
        return _RopeFn.apply(qkv if ip else qkv.contiguous(), heads, table, ip)
    return rope_qkv_reference(qkv, heads, table)
