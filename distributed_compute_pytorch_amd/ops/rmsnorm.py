"""Fused RMSNorm (gfx950 HIP kernels, csrc/kernels/rmsnorm.hip).

``y = x · rsqrt(mean(x², -1) + eps) · weight`` with fp32 statistics.
``FusedRMSNorm`` runs the hand-written kernels on a GPU for the shapes the
LayerNorm kernels take (last dim a multiple of 8, ≤ 4096; fp32 or bf16
input); under bf16 autocast an fp32 residual stream comes out as bf16 (the
cast is fused into the kernel). Everywhere else — CPU, other shapes or dtypes
— it is :func:`rms_norm_reference`, the PyTorch formula that also defines
what the kernels compute.
"""
from __future__ import annotations

import torch
from torch import nn

from .._ext import C as _C
from .linear import _acc_target, accumulating


def rms_norm_reference(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """The definition: statistics and scaling in fp32 (fp64 for fp64 input),
    rounded once to x's dtype — or to the autocast dtype for an fp32 x on a
    GPU under autocast, as the kernels do."""
    ct = torch.float64 if x.dtype == torch.float64 else torch.float32
    xf = x.to(ct)
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * weight.to(ct)
    out = x.dtype
    if x.is_cuda and x.dtype == torch.float32 and torch.is_autocast_enabled("cuda"):
        out = torch.get_autocast_dtype("cuda")
    return y.to(out)


class _RMSFn(torch.autograd.Function):
    """``dual``: also returns an alias of x as a second output — the pre-norm
    residual stream's other consumer — whose gradient the backward adds into
    dx inside the kernel (no separate add of the two gradients of x)."""

    @staticmethod
    def forward(ctx, x, weight, eps, out_dtype, dual):
        w32 = weight.detach()
        if w32.dtype != torch.float32 or not w32.is_contiguous():
            w32 = w32.float().contiguous()
        y, rstd = _C.rms_norm_fwd(x, w32, eps, out_dtype)
        ctx.save_for_backward(x, w32, rstd)
        ctx.params = (weight,)
        ctx.accum = accumulating()
        ctx.dual = dual
        if dual:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, d2=None):
        x, w32, rstd = ctx.saved_tensors
        weight = ctx.params[0]
        # under DistributedDataParallel.no_sync: dγ is added into the fp32
        # .grad by the reduction kernel (see linear.accumulate_grads_in_place)
        acc = _acc_target(ctx, weight, weight.shape) if ctx.needs_input_grad[1] else None
        dx, dw = _C.rms_norm_bwd(dy, x, w32, rstd, accumulate_into=acc, grad_residual=d2 if ctx.dual else None)
        if acc is not None or not ctx.needs_input_grad[1]:
            dw = None
        elif dw.dtype != weight.dtype:
            dw = dw.to(weight.dtype)
        return dx, dw, None, None, None


def _kernel_ok(x: torch.Tensor, weight: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and weight.is_cuda and x.dim() >= 1
            and weight.dim() == 1 and weight.shape[0] == x.shape[-1] and _C.rms_norm_supported(x.shape[-1]))


def _out_dtype(x):
    if torch.is_autocast_enabled("cuda") and x.dtype == torch.float32:
        return torch.get_autocast_dtype("cuda")  # fp32 residual stream in, bf16 out
    return None


def fused_rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    if _kernel_ok(x, weight):
        out_dtype = _out_dtype(x)
        if out_dtype in (None, torch.bfloat16):
            with torch.autocast("cuda", enabled=False):
                return _RMSFn.apply(x.contiguous(), weight, float(eps), out_dtype, False)
    return rms_norm_reference(x, weight, eps)


def fused_rms_norm_dual(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6):
    """(rms_norm(x), x) where the gradients of both outputs meet inside the
    backward kernel (pre-norm blocks: ``h, x = norm.forward_dual(x)``,
    ``x = x + f(h)``)."""
    if _kernel_ok(x, weight):
        out_dtype = _out_dtype(x)
        if out_dtype in (None, torch.bfloat16):
            with torch.autocast("cuda", enabled=False):
                return _RMSFn.apply(x.contiguous(), weight, float(eps), out_dtype, True)
    return rms_norm_reference(x, weight, eps), x


class FusedRMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float = 1e-6, device=None, dtype=None):
        super().__init__()
        self.dim, self.eps = dim, eps
        self.weight = nn.Parameter(torch.ones(dim, device=device, dtype=dtype))

    def forward(self, x):
        return fused_rms_norm(x, self.weight, self.eps)

    def forward_dual(self, x):
        """(self(x), alias of x) — see :func:`fused_rms_norm_dual`."""
        return fused_rms_norm_dual(x, self.weight, self.eps)

    def extra_repr(self):
        return f"{self.dim}, eps={self.eps}"
