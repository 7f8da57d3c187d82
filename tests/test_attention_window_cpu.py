"""Sliding-window attention off the GPU: the argument's rules are enforced in Python before any kernel call, and
the Llama decoder's two variants agree on the windowed mask."""
import pytest
import torch

from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM
from distributed_compute_pytorch_amd.ops.attention import flash_attn, flash_attn_qkv


def _models(fused_a, **kw_b):
    cfg = lambda **kw: LlamaConfig(vocab=512, n_layer=2, n_head=2, n_embd=256, ffn_hidden=256, block_size=128, **kw)
    torch.manual_seed(0)
    a, b = LlamaForCausalLM(cfg(sliding_window=48), fused=fused_a), LlamaForCausalLM(cfg(**kw_b), fused=False)
    b.load_state_dict(a.state_dict())
    return a, b, torch.randint(0, 512, (2, 64))


@pytest.mark.parametrize("C,kw,match", [(256, dict(causal=False, window=8), "causal=True"),
                                        (256, dict(causal=True, window=0), "int >= 1"),
                                        (256, dict(causal=True, window=8.0), "int >= 1"),
                                        (128, dict(causal=True, window=8), "head dim 128 only")])
def test_window_argument_errors(C, kw, match):
    q = torch.zeros(1, 64, C, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=match):
        flash_attn(q, q, q, 2, **kw)
    with pytest.raises(ValueError, match=match):
        flash_attn_qkv(torch.cat([q, q, q], -1), 2, **kw)


def test_llama_config_rejects_a_window_below_one():
    with pytest.raises(ValueError, match="sliding_window"):
        LlamaConfig(sliding_window=0)


def test_llama_window_fused_and_plain_agree_on_the_cpu():
    a, b, idx = _models(True, sliding_window=48)
    la, lb = a(idx, idx.roll(-1, 1)), b(idx, idx.roll(-1, 1))
    torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a(idx), b(idx), rtol=1e-4, atol=1e-5)
    la.backward()
    lb.backward()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-3, atol=1e-6, msg=n)


def test_llama_window_changes_logits_only_from_position_W():
    a, b, idx = _models(False)  # b: the same weights without a window
    with torch.no_grad():
        la, lb = a(idx), b(idx)
    torch.testing.assert_close(la[:, :48], lb[:, :48], rtol=1e-5, atol=1e-6)  # positions 0 … 47 see all their keys
    assert bool(((la[:, 48:] - lb[:, 48:]).abs().amax(-1) > 1e-4).all())
