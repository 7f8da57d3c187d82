"""Head dim 128 off the GPU: the Llama decoder constructs and its two variants
agree, the rotary table / reference follow the head dim, and the limits of the
128-wide attention are reported before any kernel call."""

import pytest
import torch

from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM
from distributed_compute_pytorch_amd.ops.attention import flash_attn, flash_attn_qkv
from distributed_compute_pytorch_amd.ops.rope import rope_qkv_reference, rope_table


def _cfg(**kw):
    return LlamaConfig(vocab=512, n_layer=2, n_head=2, n_embd=256, ffn_hidden=256, block_size=128, **kw)


def test_llama_d128_fused_and_plain_agree_on_the_cpu():
    torch.manual_seed(0)
    a, b = LlamaForCausalLM(_cfg(), fused=True), LlamaForCausalLM(_cfg(), fused=False)
    assert a.rope.shape == (128, 2, 64)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    idx = torch.randint(0, 512, (2, 32))
    tgt = idx.roll(-1, 1)
    la, lb = a(idx, tgt), b(idx, tgt)
    torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a(idx), b(idx), rtol=1e-4, atol=1e-5)
    la.backward()
    lb.backward()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-3, atol=1e-6, msg=n)


def test_rope_table_and_reference_at_head_dim_128():
    T, base, heads = 9, 10000.0, 2
    tab = rope_table(T, base, head_dim=128)
    assert tab.shape == (T, 2, 64) and rope_table(T, base).shape == (T, 2, 32)
    torch.manual_seed(0)
    x = torch.randn(2, T, 3 * heads * 128)
    y = rope_qkv_reference(x, heads, tab)
    ang = torch.arange(T, dtype=torch.float64)[:, None] * base ** (-torch.arange(64, dtype=torch.float64) / 64.0)
    cos, sin = ang.cos()[None, :, None, :], ang.sin()[None, :, None, :]
    a, b = x[..., :2 * heads * 128].double().reshape(2, T, 2 * heads, 128).split(64, -1)
    ref = torch.cat([a * cos - b * sin, b * cos + a * sin], -1).reshape(2, T, -1)
    torch.testing.assert_close(y[..., :2 * heads * 128].double(), ref, rtol=1e-5, atol=1e-5)
    assert torch.equal(y[..., 2 * heads * 128:], x[..., 2 * heads * 128:])


def test_d128_limits_raise_value_error():
    q = torch.zeros(1, 64, 256, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="dropout"):
        flash_attn(q, q, q, 2, dropout_p=0.1)
    with pytest.raises(ValueError, match="key-padding mask"):
        flash_attn(q, q, q, 2, key_mask=torch.ones(1, 64, dtype=torch.bool))
    with pytest.raises(ValueError, match="dropout"):
        flash_attn_qkv(torch.cat([q, q, q], -1), 2, dropout_p=0.1)
    with pytest.raises(ValueError):  # head dim 48
        LlamaForCausalLM(LlamaConfig(vocab=64, n_layer=1, n_head=2, n_embd=96, ffn_hidden=64, block_size=16))
