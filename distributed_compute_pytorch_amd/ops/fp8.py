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
* weight gradient: bf16 by default (``ops/linear.py``: in-place fp32 ``.grad``
  accumulation, micro-step deferral). The contraction runs over the rows, so
  ROW scales do not factor. With ``wgrad="fp8"`` it runs in fp8 on COLUMN
  scales, which do: ``dW[n, k] = sgy[n]·sx[k]·Σ_m qgy[m, n]·qx[m, k]``. The saved
  bf16 ``x`` (e4m3) and ``gy`` (``grad_fmt``) are quantised a second time, down
  their columns and written transposed (:func:`quantize_cols_t`), and a split-K
  fp8 GEMM with an fp32 result stores ``dW`` or adds it into ``.grad``
  (``csrc/kernels/gemm_fp8_wgrad.hip``). Under micro-step deferral, or at a
  shape that GEMM does not take, the bf16 path runs unchanged;
* bias gradient: NOT fp8, the column sums of the bf16 ``gy``.

Nothing here is a default or an autotune candidate: fp8 changes numerics.
"""
from __future__ import annotations

import torch

from .._ext import C as _C
from . import linear as _lin
from .linear import FusedLinear, _acc_target, _bias32, _linear_backward, _setup

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


def quantize_cols_t_reference(x: torch.Tensor, fmt: str = "e4m3"):
    """The recipe down the columns of ``x [M, C]``, transposed, in plain torch
    (any device): ``(q [C, Mp] float8, scale [C] fp32)``, ``Mp = ceil(M / 128) ·
    128``, the bytes ``[M, Mp)`` of every row zero. One deviation from the row
    recipe: the scale of a non-zero column is floored at the smallest normal
    fp32. A column of bf16 subnormals alone would otherwise get a subnormal
    scale, whose few bits put ``s · fmt_max`` visibly below the column's amax."""
    M, C = x.shape
    _, dtype, fmax = _fmt(fmt)
    xf = x.float().t()
    amax = xf.abs().amax(dim=-1)
    scale = torch.where(amax > 0, (amax / fmax).clamp_min(torch.finfo(torch.float32).tiny), torch.ones_like(amax))
    q = (xf / scale.unsqueeze(-1)).clamp(-fmax, fmax).to(dtype)
    out = torch.zeros(C, -(-M // 128) * 128, dtype=torch.uint8, device=x.device)
    out[:, :M] = q.view(torch.uint8)
    return out.view(q.dtype), scale


def _cols_kernel_ok(x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and 0 < x.shape[0] < 2**31
            and x.shape[1] % 64 == 0 and 0 < x.shape[1] <= 64 * 65535 and x.stride(1) == 1
            and x.data_ptr() % 16 == 0
            and (x.shape[0] <= 1 or (x.stride(0) >= x.shape[1] and x.stride(0) % 8 == 0)))


def quantize_cols_t(x: torch.Tensor, fmt: str = "e4m3"):
    """Column-wise fp8 quantisation of ``x [M, C]``, transposed and zero-padded
    to ``[C, Mp]``: the HIP kernel for bf16 GPU tensors (C a multiple of 64),
    the reference elsewhere."""
    if _cols_kernel_ok(x):
        q, s = _C.fp8_quant_cols_t(x, _fmt(fmt)[0])
        return q, s
    return quantize_cols_t_reference(x, fmt)


def fp8_weight_grad(gy: torch.Tensor, x: torch.Tensor, grad_fmt: str = "e5m2", accumulate_into=None) -> torch.Tensor:
    """``gyᵀ · x`` (fp32 ``[N, K]``) of bf16 GPU ``gy [M, N]`` and ``x [M, K]`` in
    fp8: both quantised down their columns (``gy`` in ``grad_fmt``, ``x`` in
    e4m3), multiplied on the split-K fp8 GEMM; added into ``accumulate_into``
    (a contiguous fp32 ``[N, K]`` tensor, returned) when given. Raises where the
    kernels do not take the operands."""
    if not (_cols_kernel_ok(gy) and _cols_kernel_ok(x) and gy.shape[0] == x.shape[0]
            and _C.gemm_fp8_wgrad_ok(gy.shape[1], x.shape[1], x.shape[0])):
        raise ValueError(f"fp8_weight_grad: needs bf16 GPU [M, N] and [M, K] with unit last stride, M > 0 and "
                         f"N, K multiples of 64; got {tuple(gy.shape)} and {tuple(x.shape)} on {x.device}")
    f = _fmt(grad_fmt)[0]
    return _C.gemm_fp8_wgrad(*_C.fp8_quant_cols_t(gy, f), *_C.fp8_quant_cols_t(x, 0), f,
                             accumulate_into=accumulate_into)


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
    (and, with ``weight=False``, the weight gradient) has been produced
    elsewhere: those inputs need no gradient."""

    def __init__(self, ctx, weight: bool = True):
        self._ctx = ctx
        self.needs_input_grad = (False, weight and ctx.needs_input_grad[1], ctx.needs_input_grad[2])

    def __getattr__(self, name):
        return getattr(self._ctx, name)


class _Fp8LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, w8, sw, wt8, swt, grad_fmt, wgrad_fp8=False):
        x, _, _ = _setup(ctx, x, weight, bias, weight.detach(), None)  # (no bf16 weight is needed here)
        x2 = x.reshape(-1, x.shape[-1])
        if not _kernel_ok(x2):  # rows the quantiser cannot address in place
            x2 = x2.contiguous()
        xq, sx = _C.fp8_quant_rows(x2, 0)
        y = _C.gemm_fp8(xq, sx, w8, sw, _bias32(bias) if bias is not None else None, 0)
        ctx.save_for_backward(x, wt8, swt)
        ctx.grad_fmt, ctx.wgrad_fp8 = grad_fmt, wgrad_fp8
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
        weight = ctx.params[0]
        N, K = weight.shape
        # fp8 dW, unless this weight's micro-steps are being deferred (the bf16
        # multi-segment launch owns those) or the GEMM does not take the shape
        if (ctx.wgrad_fp8 and ctx.needs_input_grad[1] and not ctx.defer and id(weight) not in _lin._PENDING
                and _C.gemm_fp8_wgrad_ok(N, K, g2.shape[0])):
            x2 = x.reshape(-1, K)
            if not _cols_kernel_ok(x2):
                x2 = x2.contiguous()
            tgt = _acc_target(ctx, weight, weight.shape)
            dw = _C.gemm_fp8_wgrad(*_C.fp8_quant_cols_t(g2, ctx.grad_fmt), *_C.fp8_quant_cols_t(x2, 0), ctx.grad_fmt,
                                   accumulate_into=tgt)
            if tgt is not None:
                dw = None  # added into weight.grad by the kernel
            elif dw.dtype != ctx.wdtype:
                dw = dw.to(ctx.wdtype)
            _, _, db = _linear_backward(_WeightGradOnly(ctx, weight=False), g2, x, None)
        else:  # dW / db: the bf16 path of ops/linear.py from the saved bf16 x and gy
            _, dw, db = _linear_backward(_WeightGradOnly(ctx), g2, x, None)
        return dx, dw, db, None, None, None, None, None, None


def _wgrad(wgrad: str) -> bool:
    if wgrad not in ("bf16", "fp8"):
        raise ValueError(f"wgrad must be 'bf16' or 'fp8', got {wgrad!r}")
    return wgrad == "fp8"


def fp8_linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, *, grad_fmt: str = "e5m2",
               w8=None, wgrad: str = "bf16") -> torch.Tensor:
    """``F.linear(x, weight, bias)`` with fp8 forward and data-gradient GEMMs
    (module docstring) as one autograd node. bf16 GPU compute only (``x`` is
    cast to bf16); ``w8``: a cached :func:`quantize_weight` result for
    ``weight``; ``wgrad="fp8"``: the weight gradient in fp8 too. Raises where the kernels do not take the shape: a missing
    kernel is an error, never a quiet fall-back."""
    N, K = weight.shape
    M = x.numel() // K if K else 0
    if not x.is_cuda or not fp8_linear_ok(M, N, K):
        raise ValueError(f"fp8_linear: needs a GPU tensor, rows > 0 and in / out features multiples of 64 "
                         f"(at most 16384); got {tuple(x.shape)} x {tuple(weight.shape)} on {x.device}")
    if w8 is None:
        w8 = quantize_weight(weight.detach().to(torch.bfloat16))
    return _Fp8LinearFn.apply(x, weight, bias, *w8, _fmt(grad_fmt)[0], _wgrad(wgrad))


class Fp8Linear(FusedLinear):
    """:class:`FusedLinear` (same constructor, same ``state_dict``) whose bf16
    GPU forward and data gradient run in fp8 (:func:`fp8_linear`), and with
    ``wgrad = "fp8"`` the weight gradient too; off that path, or at shapes the
    fp8 GEMM does not take, it is ``FusedLinear``."""

    grad_fmt = "e5m2"
    wgrad = "bf16"

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
        return _Fp8LinearFn.apply(x, self.weight, self.bias, *self._w8(*self._w16_pair()), _fmt(self.grad_fmt)[0],
                                  _wgrad(self.wgrad))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._fp8_fast(x):
            return self._forward_fp8(x)
        return super().forward(x)
