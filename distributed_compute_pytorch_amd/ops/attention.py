"""Flash attention on the hand-written MFMA kernels (``csrc/kernels/attention.hip``).

Head dim 64, bf16 activations, fp32 softmax statistics, optional causal mask
and dropout on the attention probabilities (keep decisions hashed from a
counter in the forward and kept as bits, T²/8 bytes per head, for the
backward). Replaces
``scaled_dot_product_attention`` (PyTorch-ROCm's aotriton kernels) for
GPT-2-small and BERT-base.

* :func:`flash_attn` — q, k, v as [B, T, H*64] (any row stride: slices of a
  packed projection are read in place), output [B, T, H*64] — already the
  layout the output projection consumes (no head transposes).
* :func:`flash_attn_qkv` — packed [B, T, 3*H*64] input (GPT-2's ``c_attn``);
  the backward writes dq/dk/dv straight into one packed gradient (no cat).
* :func:`pack_key_mask` — a [B, T] key-padding mask as the bits the kernels
  read (``key_mask=`` of both functions).

Key-padding mask. ``key_mask`` has the semantics of a boolean ``attn_mask`` of
shape [B, 1, 1, T] in ``scaled_dot_product_attention``: True means the key
takes part. A hidden key is excluded from the row max, the softmax normaliser
and P·V, and its dK / dV rows are exactly 0; padding positions as *queries*
are computed like any other query. The dropout decisions do not depend on the
mask. The kernels skip 64-key blocks without a visible key, and neither load
nor compute the trailing ones. Zero-row rule: a query that sees no key at all
(a fully hidden sequence, left padding under the causal mask) gets an output
row of exactly 0 and a dQ row of exactly 0 and adds nothing to dK / dV — where
a softmax over an empty set would give NaN. ``key_mask=None`` runs the kernels
that carry no mask code.

Dropout under graph capture. Every call draws a host seed (``seed=None``) and
passes it to the kernels by value, so a captured call has its seed frozen into
the graph. The forward therefore takes an optional device-resident *seed
offset* (``seed_offset=``, an int64 tensor with one element) and hashes with
``seed + offset * 0x9E3779B97F4A7C15 (mod 2^64)``, the offset read when the
kernel runs. A call with ``seed=None`` and ``dropout_p > 0`` on a capturing
stream takes the dropout counter of ``ops/dropout.py`` as its offset, the way
the Philox ops do (a snapshot + advance per call, or the counter itself inside
``batched_offsets``, whose step-end add then advances it): every replay draws
a fresh keep mask, and the calls of one replay stay independent through their
own host seeds. The backward reads the stored keep bits and needs no offset.
Eager calls skip the counter (a GPU call with dropout creates it, so that an
attention-only warm-up permits capture).
"""
from __future__ import annotations

import torch

from .._ext import C as _C
from . import dropout as _dropout

_GOLDEN64 = 0x9E3779B97F4A7C15

def _seed() -> int:
    # from torch's CPU generator: torch.manual_seed makes runs reproducible
    return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


def attn_shape_supported(T: int, C: int, heads: int) -> bool:
    """Whether the kernels take sequence length T with C = heads * 64 channels."""
    return bool(_C.attn_ok(T, C, heads))


def attn_supported(x: torch.Tensor, heads: int) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3
            and bool(_C.attn_ok(x.shape[1], x.shape[2], heads)))


def _km_args(km):
    # without a mask: exactly the _C calls (and kernels) of the unmasked op
    return () if km is None else (km,)


def _off_kwargs(off):
    return {} if off is None else {"seed_offset": off}


def _check_seed_offset(off):
    if off is None:
        return None
    if not isinstance(off, torch.Tensor):
        raise TypeError(f"seed_offset: an int64 tensor with one element required, got {type(off).__name__}")
    if off.dtype != torch.int64:
        raise TypeError(f"seed_offset: an int64 tensor required, got {off.dtype}")
    if off.numel() != 1:
        raise ValueError(f"seed_offset: a tensor with one element required, got shape {tuple(off.shape)}")
    return off


def _seed_and_offset(x, dropout_p, seed, seed_offset):
    """(host seed, device offset or None) of one call on ``x``'s device."""
    off = _check_seed_offset(seed_offset)
    if seed is not None:
        return int(seed), off
    if off is None and dropout_p > 0.0 and x.is_cuda:
        if _dropout._capturing():
            off = _dropout.take_counter(x.device)
        else:
            _dropout._ensure_counter(x.device)
    return _seed(), off


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, heads, causal, p_drop, seed, keep_bits, km, off):
        o, lse, keep = _C.flash_attn_fwd(q, k, v, heads, causal, p_drop, seed, keep_bits, *_km_args(km),
                                         **_off_kwargs(off))
        ctx.save_for_backward(q, k, v, o, lse, keep, km)
        ctx.cfg = (heads, causal, p_drop, seed)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, keep, km = ctx.saved_tensors
        heads, causal, p_drop, seed = ctx.cfg
        do = do.contiguous()
        if do.dtype != torch.bfloat16:
            do = do.to(torch.bfloat16)
        dq, dk, dv = torch.empty_like(q, memory_format=torch.contiguous_format), torch.empty_like(
            k, memory_format=torch.contiguous_format), torch.empty_like(v, memory_format=torch.contiguous_format)
        _C.flash_attn_bwd(do, q, k, v, o, lse, keep, heads, causal, p_drop, seed, dq, dk, dv, *_km_args(km))
        return dq, dk, dv, None, None, None, None, None, None, None


class _FlashAttnQKVFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, heads, causal, p_drop, seed, keep_bits, km, off):
        C = qkv.shape[2] // 3
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        o, lse, keep = _C.flash_attn_fwd(q, k, v, heads, causal, p_drop, seed, keep_bits, *_km_args(km),
                                         **_off_kwargs(off))
        ctx.save_for_backward(qkv, o, lse, keep, km)
        ctx.cfg = (heads, causal, p_drop, seed)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, keep, km = ctx.saved_tensors
        heads, causal, p_drop, seed = ctx.cfg
        do = do.contiguous()
        if do.dtype != torch.bfloat16:
            do = do.to(torch.bfloat16)
        C = qkv.shape[2] // 3
        dqkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        dq, dk, dv = dqkv[..., :C], dqkv[..., C:2 * C], dqkv[..., 2 * C:]
        _C.flash_attn_bwd(do, q, k, v, o, lse, keep, heads, causal, p_drop, seed, dq, dk, dv, *_km_args(km))
        return dqkv, None, None, None, None, None, None, None


def pack_key_mask(mask: torch.Tensor) -> torch.Tensor:
    """A key-padding mask [B, T] (bool, or an integer tensor of 0 / 1; T a
    multiple of 64; non-zero = the key takes part) as the kernels read it:
    int64 [B, 1 + T/64]. Per batch row, element 0 is the number of leading
    64-key blocks to visit (1 + the index of the last block with a visible
    key, 0 if there is none) and element 1 + j holds key block j, bit i (of
    the 64-bit pattern) = key 64j + i. The layout is internal to this module
    and the kernels. On the GPU a HIP kernel packs (no host sync, so it can be
    captured); on the CPU the same layout is built with torch ops (the
    packer's oracle)."""
    if mask.dim() != 2 or mask.shape[1] == 0 or mask.shape[1] % 64 != 0:
        raise ValueError(f"pack_key_mask: a [B, T] mask with T a multiple of 64 is required, got {tuple(mask.shape)}")
    if mask.dtype.is_floating_point or mask.dtype.is_complex:
        raise TypeError(f"pack_key_mask: bool or integer mask required, got {mask.dtype}")
    if mask.dtype != torch.bool:
        mask = mask != 0
    if mask.is_cuda:
        return _C.attn_pack_key_mask(mask.contiguous())
    B, T = mask.shape
    nblk = T // 64
    bits = mask.view(B, nblk, 64).to(torch.int64)
    # bit 63 is int64's sign bit: shifts wrap, the sum of distinct bits is their OR
    words = (bits << torch.arange(64, dtype=torch.int64)).sum(-1)
    count = ((words != 0).to(torch.int64) * torch.arange(1, nblk + 1, dtype=torch.int64)).amax(-1, keepdim=True)
    return torch.cat([count, words], dim=1)


def _packed_key_mask(key_mask, B: int, T: int):
    """``key_mask`` of flash_attn / flash_attn_qkv as the packed tensor: the
    result of :func:`pack_key_mask` is recognised by its dtype and shape
    (int64 [B, 1 + T/64]; a [B, T] mask never has that shape: T ≥ 64 >
    1 + T/64), anything else is a [B, T] mask and is packed here."""
    if key_mask is None:
        return None
    if key_mask.dtype == torch.int64 and tuple(key_mask.shape) == (B, 1 + T // 64):
        return key_mask
    if tuple(key_mask.shape) != (B, T):
        raise ValueError(f"key_mask: a [B, T] = [{B}, {T}] mask or its pack_key_mask() required, "
                         f"got {tuple(key_mask.shape)}")
    return pack_key_mask(key_mask)


def flash_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, causal: bool = False,
               dropout_p: float = 0.0, seed: int = None, key_mask: torch.Tensor = None,
               seed_offset: torch.Tensor = None) -> torch.Tensor:
    """softmax(q kᵀ / 8 [+ causal mask] [+ key mask]) → dropout(p) → · v, per head of 64.

    ``key_mask``: a [B, T] bool key-padding mask (True = the key takes part;
    module docstring), packed on the spot by one small kernel, or the result
    of :func:`pack_key_mask`. A model whose layers share one mask should pack
    it once per forward and pass the packed tensor to every layer.

    Under graph capture the op re-reads, on replay, the memory of the tensor
    it was given. Given the bool mask, the packer is part of the captured
    work: changing the mask's contents in place between replays changes the
    result accordingly (forward and backward). Given a tensor packed outside
    the capture, replays read those packed bits: later changes to the bool
    mask they were made from are not seen.

    Dropout: the keep decisions are a hash of ``seed`` (drawn from torch's CPU
    generator when None) plus ``seed_offset`` (an int64 tensor with one
    element on q's device, read by the kernel when it runs) times
    0x9E3779B97F4A7C15 (module docstring; :func:`dropout_keep_mask` is the
    oracle). With ``seed=None`` and no ``seed_offset``, a call on a capturing
    stream takes the dropout counter as its offset, so every replay draws a
    fresh mask. An explicit ``seed=`` without ``seed_offset=`` keeps its plain
    meaning: the mask is that seed's, frozen under capture, the same on every
    replay."""
    host_seed, off = _seed_and_offset(q, float(dropout_p), seed, seed_offset)
    km = _packed_key_mask(key_mask, q.shape[0], q.shape[1])
    return _FlashAttnFn.apply(q, k, v, heads, causal, float(dropout_p), host_seed, _backward_will_run(q, k, v), km,
                              off)


def flash_attn_qkv(qkv: torch.Tensor, heads: int, causal: bool = False, dropout_p: float = 0.0,
                   seed: int = None, key_mask: torch.Tensor = None, seed_offset: torch.Tensor = None) -> torch.Tensor:
    """:func:`flash_attn` on the three slices of a packed [B, T, 3*H*64]
    projection (``key_mask``, ``seed`` and ``seed_offset`` as there)."""
    host_seed, off = _seed_and_offset(qkv, float(dropout_p), seed, seed_offset)
    km = _packed_key_mask(key_mask, qkv.shape[0], qkv.shape[1])
    return _FlashAttnQKVFn.apply(qkv, heads, causal, float(dropout_p), host_seed, _backward_will_run(qkv), km, off)


def _backward_will_run(*ts) -> bool:
    """Whether the forward must keep the dropout keep bits (T²/8 bytes per
    head) for a backward: grad mode on and some input requires grad."""
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def dropout_p_effective(p: float) -> float:
    """The dropout probability the kernels apply: ``p`` rounded to a multiple
    of 1/256 (byte thresholds, as FlashAttention-2 does); kept elements are
    scaled by 1 / (1 - dropout_p_effective(p))."""
    return int(p * 256.0 + 0.5) / 256.0


def flash_attn_keep_bits(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, causal: bool,
                         dropout_p: float, seed: int, seed_offset: torch.Tensor = None) -> torch.Tensor:
    """The dropout keep decisions the forward stored for the backward, decoded
    to a bool [B, H, T, T] (test hook; ``seed_offset`` as in
    :func:`flash_attn`). Causal: entries above the diagonal are not stored
    (never read) and come back as False."""
    B, T = q.shape[0], q.shape[1]
    off = _check_seed_offset(seed_offset)
    _, _, words = _C.flash_attn_fwd(q, k, v, heads, causal, float(dropout_p), int(seed), **_off_kwargs(off))
    return decode_keep_bits(words, B, heads, T, causal)


def decode_keep_bits(words: torch.Tensor, B: int, heads: int, T: int, causal: bool) -> torch.Tensor:
    """The keep words of ``_C.flash_attn_fwd`` as a bool [B, H, T, T]."""
    nblk = T // 64
    w = words.view(B * heads, nblk, 2, T).to(torch.int64) & 0xFFFFFFFF
    kk = torch.arange(64, device=words.device)
    # key 32kh + 8g + 4hh + e of a 64-key block: word half hh, bit 8e + 4kh + g
    hh, bit = (kk >> 2) & 1, 8 * (kk & 3) + 4 * ((kk >> 5) & 1) + ((kk >> 3) & 3)
    sel = w[:, :, hh, :]                                   # [BH, nblk, 64 keys, T queries]
    bits = (sel >> bit[None, None, :, None]) & 1
    m = bits.permute(0, 3, 1, 2).reshape(B, heads, T, T).bool()
    if causal:
        m &= torch.ones(T, T, dtype=torch.bool, device=words.device).tril()
    return m


def dropout_keep_mask(B: int, H: int, T: int, p: float, seed: int, device=None, offset: int = 0) -> torch.Tensor:
    """The kernels' dropout keep-mask [B, H, T, T] rebuilt with integer torch
    ops (test oracle). ``offset``: the value of the forward's ``seed_offset``
    tensor; the hash runs on seed + offset·0x9E3779B97F4A7C15 (mod 2^64).
    Per (query q, 64-key block k, lane half hh):
    x0 = fmix32(((q << 8) | (k << 1) | hh) ^ kbh), kbh = fmix32(s0 ^
    fmix32(bh·0x9E3779B1 + s1)) (murmur3 finaliser); word j (j < 8) is
    xorshift32 (13/17/5) applied j times to x0, XOR j·0x9E3779B9; key
    64k + 32(j >> 2) + 8(j & 3) + 4hh + e takes byte e of word j and is
    kept when that byte ≥ round(256·p)."""
    M = 0xFFFFFFFF
    dev = device or "cpu"

    def mul32(x, c):  # (x * c) mod 2^32 without int64 overflow
        lo, hi = x & 0xFFFF, x >> 16
        return ((lo * c) + (((hi * c) & 0xFFFF) << 16)) & M

    def fmix32(x):
        x = x ^ (x >> 16)
        x = mul32(x, 0x85EBCA6B)
        x = x ^ (x >> 13)
        x = mul32(x, 0xC2B2AE35)
        return x ^ (x >> 16)

    def xorshift32(x):
        x = x ^ ((x << 13) & M)
        x = x ^ (x >> 17)
        return x ^ ((x << 5) & M)

    nblk = T // 64
    seed = (int(seed) + int(offset) * _GOLDEN64) & 0xFFFFFFFFFFFFFFFF
    s0, s1 = seed & M, (seed >> 32) & M
    i64 = dict(device=dev, dtype=torch.int64)
    bh = torch.arange(B * H, **i64)[:, None, None, None]
    qq = torch.arange(T, **i64)[None, :, None, None]
    kb = torch.arange(nblk, **i64)[None, None, :, None]
    hh = torch.arange(2, **i64)[None, None, None, :]
    kbh = fmix32(s0 ^ fmix32((mul32(bh, 0x9E3779B1) + s1) & M))
    x = fmix32(((qq << 8) | (kb << 1) | hh) ^ kbh)          # [BH, T, nblk, 2]
    words = []
    for j in range(8):
        words.append(x ^ ((j * 0x9E3779B9) & M))
        x = xorshift32(x)
    w = torch.stack(words, -1)                               # [BH, T, nblk, hh, j]
    e = torch.arange(4, **i64)
    r8 = (w[..., None] >> (8 * e)) & 0xFF                    # [BH, T, nblk, hh, j, e]
    thr = int(p * 256.0 + 0.5)
    keep = (r8 >= thr).reshape(B * H, T, nblk, 64)           # block offsets in (hh, j, e) order
    hv, jv, ev = torch.meshgrid(torch.arange(2), torch.arange(8), torch.arange(4), indexing="ij")
    off = (32 * (jv >> 2) + 8 * (jv & 3) + 4 * hv + ev).reshape(-1)
    inv = torch.empty_like(off)
    inv[off] = torch.arange(64)
    return keep[..., inv.to(keep.device)].reshape(B, H, T, T)
