"""The PyTorch definitions of the Llama-style ops (RMSNorm, rotary embedding,
SwiGLU) against formulas written out in fp64, and the Llama model on the CPU,
where the fused and the plain variant take the same arithmetic."""
import math

import pytest
import torch

from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM
from distributed_compute_pytorch_amd.ops.rmsnorm import FusedRMSNorm, fused_rms_norm, rms_norm_reference
from distributed_compute_pytorch_amd.ops.rope import apply_rope_qkv, rope_qkv_reference, rope_table
from distributed_compute_pytorch_amd.ops.swiglu import swiglu, swiglu_reference


@pytest.mark.parametrize("shape", [(3, 8), (2, 5, 72), (4, 100)])
def test_rms_norm_reference_matches_fp64_formula(shape):
    torch.manual_seed(0)
    x = torch.randn(shape) * 3 + 1
    w = torch.rand(shape[-1]) + 0.5
    eps = 1e-6
    xd, wd = x.double(), w.double()
    ref = xd / torch.sqrt((xd * xd).sum(-1, keepdim=True) / shape[-1] + eps) * wd
    torch.testing.assert_close(rms_norm_reference(x, w, eps).double(), ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(fused_rms_norm(x, w, eps).double(), ref, rtol=1e-5, atol=1e-6)
    # fp64 input stays fp64
    torch.testing.assert_close(rms_norm_reference(xd, wd, eps), ref, rtol=1e-12, atol=1e-12)
    m = FusedRMSNorm(shape[-1], eps)
    with torch.no_grad():
        m.weight.copy_(w)
    y, alias = m.forward_dual(x)
    torch.testing.assert_close(y.double(), ref, rtol=1e-5, atol=1e-6)
    assert alias is x
    assert list(m.state_dict()) == ["weight"]


def test_rms_norm_reference_gradients_match_fp64_formula():
    torch.manual_seed(0)
    rows, D, eps = 5, 24, 1e-6
    x = torch.randn(rows, D, dtype=torch.float64, requires_grad=True)
    w = (torch.rand(D, dtype=torch.float64) + 0.5).requires_grad_()
    g = torch.randn(rows, D, dtype=torch.float64)
    rms_norm_reference(x, w, eps).backward(g)
    xd, wd = x.detach(), w.detach()
    rstd = 1.0 / torch.sqrt((xd * xd).mean(-1, keepdim=True) + eps)
    dx = rstd * (g * wd) - xd * rstd ** 3 * (g * wd * xd).mean(-1, keepdim=True)
    dw = (g * xd * rstd).sum(0)
    torch.testing.assert_close(x.grad, dx, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(w.grad, dw, rtol=1e-10, atol=1e-12)


def test_rope_table_matches_fp64_cos_sin():
    T, base = 50, 10000.0
    tab = rope_table(T, base)
    assert tab.shape == (T, 2, 32) and tab.dtype == torch.float32
    assert rope_table(T, base) is tab  # cached
    for t in (0, 1, 7, 49):
        for i in (0, 1, 13, 31):
            ang = t * base ** (-i / 32.0)
            assert abs(float(tab[t, 0, i]) - math.cos(ang)) < 1e-7
            assert abs(float(tab[t, 1, i]) - math.sin(ang)) < 1e-7
    other = rope_table(T, 500.0)
    assert abs(float(other[3, 1, 5]) - math.sin(3 * 500.0 ** (-5 / 32.0))) < 1e-7


@pytest.mark.parametrize("heads", [1, 3])
def test_rope_reference_matches_fp64_formula(heads):
    torch.manual_seed(0)
    B, T = 2, 9
    tab = rope_table(16, 10000.0)
    qkv = torch.randn(B, T, 3 * heads * 64)
    y = apply_rope_qkv(qkv, heads, tab)  # CPU: the reference path
    ref = qkv.double().clone()
    for t in range(T):
        for hh in range(2 * heads):  # the q heads, then the k heads
            for i in range(32):
                ang = t * 10000.0 ** (-i / 32.0)
                a, b = qkv[:, t, hh * 64 + i].double(), qkv[:, t, hh * 64 + i + 32].double()
                ref[:, t, hh * 64 + i] = a * math.cos(ang) - b * math.sin(ang)
                ref[:, t, hh * 64 + i + 32] = b * math.cos(ang) + a * math.sin(ang)
    torch.testing.assert_close(y.double(), ref, rtol=1e-5, atol=1e-5)
    assert torch.equal(y[..., 2 * heads * 64:], qkv[..., 2 * heads * 64:])  # v untouched


def test_rope_then_inverse_is_identity():
    torch.manual_seed(0)
    heads, T = 2, 33
    tab = rope_table(64, 10000.0)
    qkv = torch.randn(2, T, 3 * heads * 64)
    back = rope_qkv_reference(rope_qkv_reference(qkv, heads, tab), heads, tab, inverse=True)
    # two fp32 roundings per element, |x| of a few units
    torch.testing.assert_close(back, qkv, rtol=0, atol=4 * 2.0 ** -23 * float(qkv.abs().max()))
    # the backward of the reference is that inverse rotation of the gradient
    q = qkv.clone().requires_grad_()
    g = torch.randn_like(qkv)
    rope_qkv_reference(q, heads, tab).backward(g)
    torch.testing.assert_close(q.grad, rope_qkv_reference(g, heads, tab, inverse=True), rtol=1e-5, atol=1e-6)


def test_rope_rejects_long_sequences_and_bad_widths():
    tab = rope_table(8, 10000.0)
    with pytest.raises(ValueError):
        apply_rope_qkv(torch.randn(1, 9, 192), 1, tab)
    with pytest.raises(ValueError):
        apply_rope_qkv(torch.randn(1, 4, 200), 1, tab)


@pytest.mark.parametrize("F", [8, 20])
def test_swiglu_reference_matches_fp64_formula(F):
    torch.manual_seed(0)
    p = torch.randn(7, 2 * F) * 4
    p[0, 0], p[0, 1] = 30.0, -30.0
    y = swiglu(p)
    gate, up = p[:, :F].double(), p[:, F:].double()
    ref = gate / (1.0 + torch.exp(-gate)) * up
    torch.testing.assert_close(y.double(), ref, rtol=1e-5, atol=1e-6)
    pd = p.double().requires_grad_()
    dy = torch.randn(7, F, dtype=torch.float64)
    swiglu_reference(pd).backward(dy)
    sig = 1.0 / (1.0 + torch.exp(-gate))
    d_gate = dy * up * sig * (1.0 + gate * (1.0 - sig))
    d_up = dy * gate * sig
    torch.testing.assert_close(pd.grad, torch.cat([d_gate, d_up], -1), rtol=1e-10, atol=1e-12)


def _tiny(**kw):
    return LlamaConfig(vocab=512, n_layer=2, n_head=2, n_embd=128, ffn_hidden=256, block_size=128, **kw)


@pytest.mark.parametrize("tie", [False, True])
def test_fused_and_plain_models_share_state_dict_and_loss(tie):
    torch.manual_seed(0)
    a = LlamaForCausalLM(_tiny(tie_embeddings=tie), fused=True)
    b = LlamaForCausalLM(_tiny(tie_embeddings=tie), fused=False)
    assert list(a.state_dict()) == list(b.state_dict())
    keys = set(a.state_dict())
    for k in ("tok_embeddings.weight", "norm.weight", "output.weight", "layers.1.attention_norm.weight",
              "layers.0.ffn_norm.weight", "layers.0.attention.wq.weight", "layers.0.attention.wk.weight",
              "layers.0.attention.wv.weight", "layers.1.attention.wo.weight", "layers.0.feed_forward.w1.weight",
              "layers.0.feed_forward.w2.weight", "layers.1.feed_forward.w3.weight"):
        assert k in keys, k
    assert not any("rope" in k or "bias" in k for k in keys)
    b.load_state_dict(a.state_dict())
    a.load_state_dict(b.state_dict())
    idx = torch.randint(0, 512, (2, 32))
    tgt = idx.roll(-1, 1)
    la, lb = a(idx, tgt), b(idx, tgt)
    assert abs(float(la.detach()) - math.log(512)) < 0.5  # random init: near-uniform predictions
    torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a(idx), b(idx), rtol=1e-4, atol=1e-5)
    la.backward()
    lb.backward()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-3, atol=1e-6, msg=n)


def test_model_loss_decreases():
    torch.manual_seed(0)
    m = LlamaForCausalLM(_tiny(), fused=True)
    opt = torch.optim.AdamW(m.parameters(), lr=3e-3)
    idx = torch.randint(0, 512, (4, 32))
    tgt = idx.roll(-1, 1)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = m(idx, tgt)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0] - 0.5, losses


def test_model_rejects_other_head_dims_and_long_sequences():
    with pytest.raises(ValueError):
        LlamaForCausalLM(LlamaConfig(vocab=64, n_layer=1, n_head=2, n_embd=96, ffn_hidden=64, block_size=16))
    m = LlamaForCausalLM(LlamaConfig(vocab=64, n_layer=1, n_head=1, n_embd=64, ffn_hidden=64, block_size=16))
    with pytest.raises(ValueError):
        m(torch.zeros(1, 17, dtype=torch.long))
