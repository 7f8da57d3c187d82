"""Opt-in fp8 Linear: row-scaled OCP e4m3 / e5m2 operands on gfx950's
``v_mfma_scale_f32_32x32x64_f8f6f4`` (``csrc/kernels/gemm_fp8.hip``).

Recipe (row-wise, no global amax, no host sync, deterministic): every row of an
operand gets its own fp32 scale ``s = amax(row) / fmt_max`` (1 for an all-zero
row) and is stored as ``cvt_fp8(clamp(x / s, ±fmt_max))``, round-to-nearest-even.
The scales factor out of the contraction, so the GEMM runs on the raw fp8 codes
and its epilogue multiplies by ``sa[m] · sb[n]`` in fp32.

* forward: ``y = q(x) · q(W)ᵀ`` — both e4m3, W quantised along its input axis;
* data gradient: ``dx = q(gy) · q(Wᵀ)ᵀ`` — ``gy`` in ``grad_fmt`` (e5m2 by
  default), ``Wᵀ`` a second e4m3 copy quantised along the output axis;
* weight / bias gradient: NOT fp8. The contraction runs over the rows, each
  with its own scale, so it does not factor; it stays on the bf16 kernels of
  ``ops/linear.py`` (same in-place fp32 ``.grad`` accumulation and deferral).

Nothing here is a default or an autotune candidate: fp8 changes numerics.
"""
from __future__ import annotations

import torch

from .._ext import C as _C
from .linear import FusedLinear, _bias32, _linear_backward, _setup

_FMT = {"e4m3": (0, torch.float8_e4m3fn, 448.0), "e5m2": (1, torch.float8_e5m2, 57344.0)}


def _fmt(fmt: str):
    try:
        return _FMT[fmt]
    except KeyError:
        raise ValueError(f"fp8 format must be 'e4m3' or 'e5m2', got {fmt!r}") from None


def quantize_rows_reference(x: torch.Tensor, fmt: str = "e4m3"):
    """The recipe in plain torch (any device): ``(q [R, K] float8, scale [R] fp32)``."""
    _, dtype, fmax = _fmt(fmt)
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    scale = torch.where(amax > 0, amax / fmax, torch.ones_like(amax))
    q = (xf / scale.unsqueeze(-1)).clamp(-fmax, fmax).to(dtype)
    return q, scale


def _kernel_ok(x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.shape[1] % 16 == 0
            and 0 < x.shape[1] <= 16384 and x.stride(1) == 1 and x.data_ptr() % 16 == 0
            and (x.shape[0] <= 1 or (x.stride(0) >= x.shape[1] and x.stride(0) % 8 == 0)))


def quantize_rows(x: torch.Tensor, fmt: str = "e4m3"):
    """Row-wise fp8 quantisation of a 2-D tensor: the HIP kernel for bf16 GPU
    rows (K a multiple of 16, at most 16384), the reference elsewhere."""
    if _kernel_ok(x):
        q, s = _C.fp8_quant_rows(x, _fmt(fmt)[0])
        return q, s
    return quantize_rows_reference(x, fmt)


def quantize_weight(w16: torch.Tensor, w16t: torch.Tensor | None = None):
    """The fp8 pair of a bf16 weight [N, K]: ``(W8 [N, K], sw [N], Wᵀ8 [K, N],
    swt [K])``, both e4m3 (``w16t``: the bf16 Wᵀ where the caller has it)."""
    if w16t is None:
        w16t = w16.t().contiguous()
    return quantize_rows(w16, "e4m3") + quantize_rows(w16t, "e4m3")


def fp8_linear_ok(M: int, N: int, K: int) -> bool:
    """Shapes the fp8 forward ([M, K] · [N, K]ᵀ) and data gradient ([M, N] ·
    [K, N]ᵀ) both take: N and K multiples of 64, at most 16384."""
    return (M > 0 and max(N, K) <= 16384 and N % 16 == 0 and K % 16 == 0 and _C.gemm_fp8_ok(M, N, K)
            and _C.gemm_fp8_ok(M, K, N))


class _WeightGradOnly:
    """The autograd ctx as ``_linear_backward`` sees it when the data gradient
    has been produced elsewhere: input 0 needs no gradient."""

    def __init__(self, ctx):
        self._ctx = ctx
        self.needs_input_grad = (False,) + tuple(ctx.needs_input_grad[1:3])

    def __getattr__(self, name):
        return getattr(self._ctx, name)


class _Fp8LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, w8, sw, wt8, swt, grad_fmt):
        x, _, _ = _setup(ctx, x, weight, bias, weight.detach(), None)  # (no bf16 weight is needed here)
        x2 = x.reshape(-1, x.shape[-1])
        if not _kernel_ok(x2):  # rows the quantiser cannot address in place
            x2 = x2.contiguous()
        xq, sx = _C.fp8_quant_rows(x2, 0)
        y = _C.gemm_fp8(xq, sx, w8, sw, _bias32(bias) if bias is not None else None, 0)
        ctx.save_for_backward(x, wt8, swt)
        ctx.grad_fmt = grad_fmt
        return y.view(*x.shape[:-1], w8.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x, wt8, swt = ctx.saved_tensors
        gy = gy.contiguous()
        if gy.dtype != torch.bfloat16:
            gy = gy.to(torch.bfloat16)
        g2 = gy.view(-1, gy.shape[-1])
        dx = None
        if ctx.needs_input_grad[0]:
            gq, sg = _C.fp8_quant_rows(g2, ctx.grad_fmt)
            dx = _C.gemm_fp8(gq, sg, wt8, swt, None, ctx.grad_fmt).view(x.shape)
        # dW / db: the bf16 path of ops/linear.py from the saved bf16 x and gy
        _, dw, db = _linear_backward(_WeightGradOnly(ctx), g2, x, None)
        return dx, dw, db, None, None, None, None, None


def fp8_linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, *, grad_fmt: str = "e5m2",
               w8=None) -> torch.Tensor:
    """``F.linear(x, weight, bias)`` with fp8 forward and data-gradient GEMMs
    (module docstring) as one autograd node. bf16 GPU compute only (``x`` is
    cast to bf16); ``w8``: a cached :func:`quantize_weight` result for
    ``weight``. Raises where the kernels do not take the shape: a missing
    kernel is an error, never a quiet fall-back."""
    N, K = weight.shape
    M = x.numel() // K if K else 0
    if not x.is_cuda or not fp8_linear_ok(M, N, K):
        raise ValueError(f"fp8_linear: needs a GPU tensor, rows > 0 and in / out features multiples of 64 "
                         f"(at most 16384); got {tuple(x.shape)} x {tuple(weight.shape)} on {x.device}")
    if w8 is None:
        w8 = quantize_weight(weight.detach().to(torch.bfloat16))
    return _Fp8LinearFn.apply(x, weight, bias, *w8, _fmt(grad_fmt)[0])


class Fp8Linear(FusedLinear):
    """:class:`FusedLinear` (same constructor, same ``state_dict``) whose bf16
    GPU forward and data gradient run in fp8 (:func:`fp8_linear`); off that
    path, or at shapes the fp8 GEMM does not take, it is ``FusedLinear``."""

    grad_fmt = "e5m2"

    def _w8(self, w16: torch.Tensor, w16t: torch.Tensor):
        """The fp8 weight pair, re-quantised only when the weight has changed
        (the key of ``FusedLinear._bf16``); never cached during graph capture."""
        if torch.cuda.is_current_stream_capturing():
            return quantize_weight(w16, w16t)
        from ..optim.fused import param_epoch

        p = self.weight
        key = (p._version, param_epoch(), p.data_ptr())
        c = self.__dict__.get("_w8_cache")
        if c is not None and c[0] == key:
            return c[1]
        t = quantize_weight(w16, w16t)
        self.__dict__["_w8_cache"] = (key, t)
        return t

    def _fp8_fast(self, x: torch.Tensor) -> bool:
        return (self._fast(x) and x.numel() > 0
                and fp8_linear_ok(x.numel() // self.in_features, self.out_features, self.in_features))

    def _forward_fp8(self, x: torch.Tensor) -> torch.Tensor:
        return _Fp8LinearFn.apply(x, self.weight, self.bias, *self._w8(*self._w16_pair()), _fmt(self.grad_fmt)[0])

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._fp8_fast(x):
            return self._forward_fp8(x)
        return super().forward(x)
