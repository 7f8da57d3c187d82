"""Sliding-window causal attention in the head-dim-128 flash kernels (csrc/kernels/attention_d128.hip, WIN) on
the GPU against a plain fp64 reference; inputs and bounds of tests/test_gpu_attention_d128.py. What each shape
reaches and the worst fractions of the bounds seen on an MI355X (printed by the tests): NOTES §49."""
import math

import pytest
import torch
from test_gpu_attention_d128 import BF, D, _inputs  # the same inputs recipe

from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM
from distributed_compute_pytorch_amd.ops.attention import attn_supported, flash_attn, flash_attn_qkv

pytestmark = pytest.mark.gpu


def _ref64(q, k, v, do, H, W):
    """softmax(q kᵀ / sqrt(128)) v over keys i − W < j ≤ i, per head, in fp64: (o, P·|v|, dq, dk, dv) as [B, T, H*128]."""
    B, T, _ = q.shape
    q64, k64, v64 = (t.double().view(B, T, H, D).transpose(1, 2).detach().requires_grad_() for t in (q, k, v))
    i = torch.arange(T, device=q.device)
    hidden = (i[None, :] > i[:, None]) | (i[None, :] <= i[:, None] - W)
    p = (q64 @ k64.transpose(-1, -2) / math.sqrt(D)).masked_fill(hidden, float("-inf")).softmax(-1)
    o = p @ v64
    dq, dk, dv = torch.autograd.grad(o, (q64, k64, v64), do.double().view(B, T, H, D).transpose(1, 2))
    flat = lambda t: t.detach().transpose(1, 2).reshape(B, T, H * D)
    return flat(o), flat(p.detach() @ v64.detach().abs()), flat(dq), flat(dk), flat(dv)


def _run(dev, B, H, T, qscale, seed=0, **kw):
    q, k, v, do = _inputs(dev, B, H, T, qscale, seed)
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    o = flash_attn(q, k, v, H, causal=True, **kw)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


@pytest.mark.parametrize("B,H,T,W,qscale", [(1, 1, 128, 64, 1), (1, 1, 128, 32, 1), (1, 2, 192, 17, 4),
                                            (1, 2, 320, 100, 1), (2, 2, 256, 128, 4), (1, 1, 320, 191, 1),
                                            (3, 43, 256, 96, 1), (1, 1, 64, 63, 1)])
def test_flash_attn_window_matches_fp64(cuda, B, H, T, W, qscale):
    o_ref, pabsv, *g_ref = _ref64(*_inputs(cuda, B, H, T, qscale), H, W)
    o, *g = _run(cuda, B, H, T, qscale, window=W)
    frac = float(((o.double() - o_ref).abs() / (2.0 ** -8 * (o_ref.abs() + pabsv) + 1e-6)).max())
    rels = [float((a.double() - r).norm() / r.norm()) for a, r in zip([o, *g], [o_ref, *g_ref])]
    print(f"window B{B} H{H} T{T} W{W} qscale={qscale}: fwd bound fraction {frac:.3f}, "
          f"rel L2 o {rels[0]:.2e} dq {rels[1]:.2e} dk {rels[2]:.2e} dv {rels[3]:.2e}")
    assert frac <= 1.0
    assert rels[0] < 1e-2 and max(rels[1:]) < 2e-2, rels


def test_flash_attn_window_of_one_key(cuda):
    """W = 1: P is the identity, so o = v and dv = do exactly; dq and dk are (dP − δ)·k and (dP − δ)·q with dP and
    δ two fp32 sums of the same 128 exact products in different orders: zero up to twice the summation error."""
    H, T = 2, 192
    q, k, v, do = _inputs(cuda, 1, H, T, 1)
    o, dq, dk, dv = _run(cuda, 1, H, T, 1, window=1)
    assert torch.equal(o, v) and torch.equal(dv, do)
    heads = lambda t: t.double().view(T, H, D)
    eps = 2 * 128 * 2.0 ** -24 * (heads(do) * heads(v)).abs().sum(-1, keepdim=True) / math.sqrt(D)
    for g, other in ((dq, k), (dk, q)):
        frac = float((heads(g).abs() / (eps * heads(other).abs().amax(-1, keepdim=True))).max())
        print(f"window 1: worst fraction of the summation-error bound {frac:.3f}")
        assert torch.isfinite(g).all() and frac <= 1.0


# W ≥ T is plain causal attention, bit for bit; two windowed runs are bitwise equal
@pytest.mark.parametrize("T,kw,kw2", [(192, dict(window=192), {}), (192, dict(window=197), {}),
                                      (320, dict(window=100), dict(window=100))])
def test_flash_attn_window_bitwise(cuda, T, kw, kw2):
    assert all(torch.equal(a, b) for a, b in zip(_run(cuda, 1, 2, T, 4, seed=2, **kw), _run(cuda, 1, 2, T, 4, seed=2, **kw2)))


def test_flash_attn_qkv_window_packed_equals_slices(cuda):
    q, k, v, do = _inputs(cuda, 2, 2, 192, 1, seed=1)
    qkv = torch.cat([q, k, v], -1).requires_grad_()
    o = flash_attn_qkv(qkv, 2, causal=True, window=100)
    o.backward(do)
    o2, *g = _run(cuda, 2, 2, 192, 1, seed=1, window=100)
    assert torch.equal(o, o2) and torch.equal(qkv.grad, torch.cat(g, -1))


def test_llama_window_fused_matches_plain_fp32(cuda):
    """fused=True under bf16 autocast (windowed flash kernels) against the plain fp32 model (SDPA with the bool
    mask); noise floor: the plain model's own bf16-autocast run (err < 4·noise + 2e-2)."""
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab=512, n_layer=2, n_head=2, n_embd=256, ffn_hidden=256, block_size=128, sliding_window=48)
    assert attn_supported(torch.empty(2, 128, 768, device=cuda, dtype=BF)[..., :256], 2, head_dim=128)
    fused, plain = LlamaForCausalLM(cfg, fused=True).to(cuda), LlamaForCausalLM(cfg, fused=False).to(cuda)
    plain.load_state_dict(fused.state_dict())
    idx = torch.randint(0, 512, (2, 128), device=cuda)

    def run(m, amp):
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF, enabled=amp):
            loss = m(idx, idx.roll(-1, 1))
        loss.backward()
        return float(loss.detach()), {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}

    (l_ref, g_ref), (l_noise, g_noise), (l_fused, g_fused) = run(plain, False), run(plain, True), run(fused, True)
    assert abs(l_fused - l_ref) < 4 * abs(l_noise - l_ref) + 2e-2 * max(1.0, abs(l_ref)), (l_fused, l_noise, l_ref)
    for n, r in g_ref.items():
        den = float(r.norm().clamp_min(1e-3))
        err, noise = float((g_fused[n] - r).norm()) / den, float((g_noise[n] - r).norm()) / den
        print(f"{n}: fused err {err:.3e} plain-bf16 noise {noise:.3e}")
        assert err < 4 * noise + 2e-2, (n, err, noise)
