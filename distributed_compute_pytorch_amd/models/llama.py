"""Llama-style decoder: RMSNorm, rotary position embedding, SwiGLU MLP,
bias-free Linears, pre-norm residual blocks, causal attention.

``llama_small()``: 12 layers, d_model 768, 12 heads of 64, SwiGLU hidden 2048,
context 1024, vocabulary 32000, untied head. Random init (std 0.02, residual
projections scaled by 1/sqrt(2·n_layer)). Parameter names follow the usual
Llama layout (``tok_embeddings``, ``layers.N.attention.wq`` …
``layers.N.feed_forward.w1 / w3 / w2``, ``layers.N.attention_norm``,
``layers.N.ffn_norm``, ``norm``, ``output``): a ``fused=False`` model loads a
``fused=True`` state dict and back.

Block: ``x += wo(attn(rope(qkv(attention_norm(x)))))``,
``x += w2(swiglu(w1|w3(ffn_norm(x))))``; a final norm, then the head.

MI355X path (``fused=True`` on a GPU under bf16 autocast): ``wq / wk / wv``
run as one packed GEMM and ``w1 / w3`` as another (bf16 operands from the
model's ``LinearWeightPrep``); RMSNorm, rotary embedding (in place on the
packed projection) and SwiGLU are the hand-written kernels of
``ops/rmsnorm.py``, ``ops/rope.py``, ``ops/swiglu.py``; attention is the MFMA
flash attention on the packed projection; the residual stream's two gradients
meet inside the RMSNorm backward kernel (``forward_dual``); head + loss is
``lm_head_cross_entropy``. The Linear kernels' epilogues take an fp32 bias, so
the bias-free Linears hand them a cached all-zero one (never a parameter, no
gradient). ``fused=False`` is plain PyTorch (``scaled_dot_product_attention``,
``F.silu``); on the CPU both variants take that arithmetic.

Out of scope: grouped-query attention (the attention kernels take equal q and
k head counts), head dims other than 64, KV-cache decoding.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
from torch import nn
from torch.nn import functional as F

from ..ops.attention import attn_supported, flash_attn_qkv
from ..ops.dropout import dropout_add
from ..ops.embedding import FusedEmbedding
from ..ops.linear import FusedLinear, LinearWeightPrep, _LinearFn, _PackedLinearFn, packed_linear, prepped_linear
from ..ops.lm_head import lm_head_cross_entropy, padded_vocab
from ..ops.rmsnorm import FusedRMSNorm
from ..ops.rope import apply_rope_qkv, rope_qkv_reference, rope_table
from ..ops.swiglu import swiglu


@dataclass
class LlamaConfig:
    vocab: int = 32000
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 768
    ffn_hidden: int = 2048
    block_size: int = 1024
    rope_base: float = 10000.0
    dropout: float = 0.0
    tie_embeddings: bool = False
    norm_eps: float = 1e-6


_ZERO_BIAS: dict = {}


def _zero_bias(n: int, device):
    """(fp32, bf16) all-zero bias of n outputs, cached per device: what the
    GEMM epilogues (fp32) and the hipBLASLt candidate (bf16) take in place of
    a bias these Linears do not have."""
    key = (n, device)
    z = _ZERO_BIAS.get(key)
    if z is None:
        z32 = torch.zeros(n, device=device, dtype=torch.float32)
        z = _ZERO_BIAS[key] = (z32, z32.to(torch.bfloat16))
    return z


def _bf16_compute(x: torch.Tensor) -> bool:
    return x.is_cuda and (x.dtype == torch.bfloat16 or (torch.is_autocast_enabled("cuda")
                                                        and torch.get_autocast_dtype("cuda") == torch.bfloat16))


class BiasFreeLinear(FusedLinear):
    """``FusedLinear(bias=False)`` whose bf16 GPU path still reaches the
    autotuned GEMM kernels (they want a bias operand: the cached zero one)."""

    def __init__(self, in_features: int, out_features: int):
        super().__init__(in_features, out_features, bias=False)

    def forward(self, x):
        if self._fast(x):
            w16, w16t = self._w16_pair()
            z32, z16 = _zero_bias(self.out_features, x.device)
            return _LinearFn.apply(x, self.weight, z32, w16, z16, w16t)
        return F.linear(x, self.weight)


def _packed_bias_free(x: torch.Tensor, layers) -> torch.Tensor:
    """``packed_linear`` for bias-free layers: the same one-GEMM node, handed
    the zero bias; off the bf16 GPU path it is ``packed_linear`` itself."""
    if _bf16_compute(x) and all(l.in_features % 8 == 0 and l.out_features % 8 == 0 for l in layers):
        z32, _ = _zero_bias(sum(l.out_features for l in layers), x.device)
        v = prepped_linear(tuple(l.weight for l in layers))
        if v is not None:
            return _PackedLinearFn.apply(x, z32, v[0], v[1], *(l.weight for l in layers))
        w = torch.cat([l.weight for l in layers], 0)
        w16 = w.detach().to(torch.bfloat16)
        return _LinearFn.apply(x, w, z32, w16, None, w16.t().contiguous())
    return packed_linear(x, layers)


class RMSNorm(nn.Module):
    """The plain-PyTorch RMSNorm of the ``fused=False`` model."""

    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps) * self.weight.float()).to(x.dtype)


class Attention(nn.Module):
    def __init__(self, cfg: LlamaConfig, fused: bool):
        super().__init__()
        lin = BiasFreeLinear if fused else (lambda i, o: nn.Linear(i, o, bias=False))
        C = cfg.n_embd
        self.wq, self.wk, self.wv, self.wo = lin(C, C), lin(C, C), lin(C, C), lin(C, C)
        self.n_head, self.dropout, self.fused = cfg.n_head, cfg.dropout, fused

    def forward(self, x, table):
        B, T, C = x.shape
        h = self.n_head
        p = self.dropout if self.training else 0.0
        if self.fused:
            qkv = _packed_bias_free(x, (self.wq, self.wk, self.wv))
            if attn_supported(qkv[..., :C], h) and table.is_cuda and table.dtype == torch.float32:
                # rotated in place on the GEMM's output, read in place by the
                # MFMA flash attention: no head transposes, one packed gradient
                qkv = apply_rope_qkv(qkv, h, table, inplace=True)
                return self.wo(flash_attn_qkv(qkv, h, causal=True, dropout_p=p))
        else:
            qkv = torch.cat([self.wq(x), self.wk(x), self.wv(x)], -1)
        q, k, v = rope_qkv_reference(qkv, h, table).split(C, dim=2)
        q = q.view(B, T, h, 64).transpose(1, 2)
        k = k.view(B, T, h, 64).transpose(1, 2)
        v = v.view(B, T, h, 64).transpose(1, 2)
        y = F.scaled_dot_product_attention(q, k, v, dropout_p=p, is_causal=True)
        return self.wo(y.transpose(1, 2).contiguous().view(B, T, C))


class FeedForward(nn.Module):
    def __init__(self, cfg: LlamaConfig, fused: bool):
        super().__init__()
        lin = BiasFreeLinear if fused else (lambda i, o: nn.Linear(i, o, bias=False))
        self.w1 = lin(cfg.n_embd, cfg.ffn_hidden)  # gate
        self.w3 = lin(cfg.n_embd, cfg.ffn_hidden)  # up
        self.w2 = lin(cfg.ffn_hidden, cfg.n_embd)  # down
        self.fused = fused

    def forward(self, x):
        if self.fused:
            return self.w2(swiglu(_packed_bias_free(x, (self.w1, self.w3))))
        return self.w2(F.silu(self.w1(x)) * self.w3(x))


def _plain_dropout_add(x, residual, p, training):
    return residual + F.dropout(x, p, training)


class Block(nn.Module):
    def __init__(self, cfg: LlamaConfig, fused: bool):
        super().__init__()
        norm = FusedRMSNorm if fused else RMSNorm
        self.attention_norm = norm(cfg.n_embd, cfg.norm_eps)
        self.attention = Attention(cfg, fused)
        self.ffn_norm = norm(cfg.n_embd, cfg.norm_eps)
        self.feed_forward = FeedForward(cfg, fused)
        self.p, self.fused = cfg.dropout, fused

    def forward(self, x, table):
        if self.fused:
            # dual-output norm: the residual stream's two gradients (branch +
            # skip) are summed inside the RMSNorm backward kernel
            h, x = self.attention_norm.forward_dual(x)
            x = dropout_add(self.attention(h, table), x, self.p, self.training)
            h, x = self.ffn_norm.forward_dual(x)
            return dropout_add(self.feed_forward(h), x, self.p, self.training)
        x = _plain_dropout_add(self.attention(self.attention_norm(x), table), x, self.p, self.training)
        return _plain_dropout_add(self.feed_forward(self.ffn_norm(x)), x, self.p, self.training)


class LlamaForCausalLM(nn.Module):
    def __init__(self, cfg: LlamaConfig = LlamaConfig(), fused: bool = True):
        super().__init__()
        if cfg.n_embd != 64 * cfg.n_head:
            raise ValueError(f"LlamaForCausalLM: head dim 64 required (n_embd = 64 * n_head), got n_embd "
                             f"{cfg.n_embd} with {cfg.n_head} heads")
        self.cfg, self.fused = cfg, fused
        self.tok_embeddings = (FusedEmbedding if fused else nn.Embedding)(cfg.vocab, cfg.n_embd)
        self.drop = nn.Dropout(cfg.dropout)
        self.layers = nn.ModuleList([Block(cfg, fused) for _ in range(cfg.n_layer)])
        self.norm = (FusedRMSNorm if fused else RMSNorm)(cfg.n_embd, cfg.norm_eps)
        # a plain module either way: the head runs through lm_head_cross_entropy
        # on the padded bf16 copy the LinearWeightPrep keeps (``heads=``)
        self.output = nn.Linear(cfg.n_embd, cfg.vocab, bias=False)
        # cos / sin of every position, fp32 [block_size, 2, 32]; not a state_dict entry
        self.register_buffer("rope", rope_table(cfg.block_size, cfg.rope_base).clone(), persistent=False)
        self.apply(self._init)
        for n, p in self.named_parameters():
            if n.endswith("wo.weight") or n.endswith("w2.weight"):
                nn.init.normal_(p, 0.0, 0.02 / math.sqrt(2 * cfg.n_layer))
        if cfg.tie_embeddings:
            self.output.weight = self.tok_embeddings.weight

    @staticmethod
    def _init(m):
        if isinstance(m, (nn.Linear, nn.Embedding)):
            nn.init.normal_(m.weight, 0.0, 0.02)

    def _packed_groups(self):
        g = [(b.attention.wq.weight, b.attention.wk.weight, b.attention.wv.weight) for b in self.layers]
        return g + [(b.feed_forward.w1.weight, b.feed_forward.w3.weight) for b in self.layers]

    def forward(self, idx, targets=None):
        B, T = idx.shape
        if T > self.cfg.block_size:
            raise ValueError(f"sequence length {T} exceeds block_size {self.cfg.block_size}")
        if self.fused and idx.is_cuda:
            # bf16 W / Wᵀ of every Linear, the packed groups and the padded head: one launch per optimizer step
            LinearWeightPrep.attach(self, packed=self._packed_groups(),
                                    heads={self.output.weight: padded_vocab(self.cfg.vocab)})
        x = self.drop(self.tok_embeddings(idx))
        for blk in self.layers:
            x = blk(x, self.rope)
        x = self.norm(x)
        if targets is not None and self.fused:
            # head + cross-entropy as one node on our GEMMs (no logits returned)
            return lm_head_cross_entropy(x, self.output.weight, None, targets)
        logits = F.linear(x, self.output.weight)
        if targets is None:
            return logits
        return F.cross_entropy(logits.view(B * T, -1).float(), targets.reshape(-1))


def llama_small(fused: bool = True, **kw) -> LlamaForCausalLM:
    return LlamaForCausalLM(LlamaConfig(**kw), fused=fused)
