"""Head-dim-128 flash attention (csrc/kernels/attention_d128.hip), rotary
embedding at 128 and the Llama decoder at that width, on the GPU, against
plain fp64 references written here.

Worst fractions of the bounds seen on an MI355X (printed by the tests): see
NOTES §44."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D = 128


def _inputs(dev, B, H, T, qscale, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q, k, v, do = (torch.randn(B, T, H * D, generator=g) for _ in range(4))
    return [t.to(dev).to(BF) for t in (q * qscale, k, v, do)]


def _ref64(q, k, v, do, H, causal):
    """softmax(q kᵀ / sqrt(128)) v per head in fp64: (o, P·|v|, dq, dk, dv), all [B, T, H*128]."""
    B, T, _ = q.shape
    q64, k64, v64 = (t.double().view(B, T, H, D).transpose(1, 2).detach().requires_grad_() for t in (q, k, v))
    s = q64 @ k64.transpose(-1, -2) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    p = s.softmax(-1)
    o = p @ v64
    dq, dk, dv = torch.autograd.grad(o, (q64, k64, v64), do.double().view(B, T, H, D).transpose(1, 2))
    flat = lambda t: t.detach().transpose(1, 2).reshape(B, T, H * D)
    return flat(o), flat(p.detach() @ v64.detach().abs()), flat(dq), flat(dk), flat(dv)


def _rel(a, r):
    return float((a.double() - r).norm() / r.norm())


# the last case puts 258 workgroups in the causal grid: two serpentine rounds
@pytest.mark.parametrize("B,H,T,causal,qscale", [(1, 1, 64, False, 1), (1, 1, 64, True, 1), (2, 3, 128, True, 1),
                                                 (1, 2, 192, False, 1), (1, 2, 192, True, 4), (1, 2, 320, True, 1),
                                                 (2, 2, 256, False, 4), (3, 43, 256, True, 1)])
def test_flash_attn_d128_matches_fp64(cuda, B, H, T, causal, qscale):
    from distributed_compute_pytorch_amd.ops.attention import flash_attn

    q, k, v, do = _inputs(cuda, B, H, T, qscale)
    o_ref, pabsv, dq_ref, dk_ref, dv_ref = _ref64(q, k, v, do, H, causal)
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    o = flash_attn(q, k, v, H, causal=causal)
    o.backward(do)
    # 2^-9 for the output's rounding + 2^-9 per probability for the bf16 P operand, doubled
    bound = 2.0 ** -8 * (o_ref.abs() + pabsv) + 1e-6
    frac = float(((o.detach().double() - o_ref).abs() / bound).max())
    rels = [_rel(o.detach(), o_ref), _rel(q.grad, dq_ref), _rel(k.grad, dk_ref), _rel(v.grad, dv_ref)]
    print(f"d128 B{B} H{H} T{T} causal={causal} qscale={qscale}: fwd bound fraction {frac:.3f}, "
          f"rel L2 o {rels[0]:.2e} dq {rels[1]:.2e} dk {rels[2]:.2e} dv {rels[3]:.2e}")
    assert frac <= 1.0
    assert rels[0] < 1e-2 and max(rels[1:]) < 2e-2, rels


def test_flash_attn_qkv_d128_packed_equals_slices(cuda):
    from distributed_compute_pytorch_amd.ops.attention import flash_attn, flash_attn_qkv

    H, C = 2, 2 * D
    q, k, v, do = _inputs(cuda, 2, H, 192, 1, seed=1)
    qkv = torch.cat([q, k, v], -1).requires_grad_()
    o = flash_attn_qkv(qkv, H, causal=True)
    o.backward(do)
    parts = [t.clone().requires_grad_() for t in (q, k, v)]
    o2 = flash_attn(*parts, H, causal=True)
    o2.backward(do)
    assert torch.equal(o, o2)
    assert torch.equal(qkv.grad, torch.cat([t.grad for t in parts], -1))


def test_flash_attn_d128_is_deterministic(cuda):
    from distributed_compute_pytorch_amd.ops.attention import flash_attn

    def run():
        q, k, v, do = _inputs(cuda, 1, 2, 320, 4, seed=2)
        q, k, v = (t.requires_grad_() for t in (q, k, v))
        o = flash_attn(q, k, v, 2, causal=True)
        o.backward(do)
        return o.detach(), q.grad, k.grad, v.grad

    assert all(torch.equal(a, b) for a, b in zip(run(), run()))


def _bf16_key(t):  # bf16 values as integers in value order
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def _within_one_bf16_ulp(got, ref64):
    """got is the fp64 value rounded once to bf16, or a neighbour of it."""
    k0 = _bf16_key(ref64.float().to(BF))
    cands = torch.stack([k0 - 1, k0, k0 + 1])
    vals = torch.where(cands >= 0, cands, -cands - 32768).to(torch.int16).view(BF).double()
    kr = cands.gather(0, (vals - ref64.unsqueeze(0)).abs().argmin(0, keepdim=True))[0]
    return int((_bf16_key(got) - kr).abs().max()) <= 1


def _rope64(x, heads, table, sign=1.0):
    B, T, _ = x.shape
    cos, sin = table[:T, 0].double()[None, :, None, :], sign * table[:T, 1].double()[None, :, None, :]
    a, b = x[..., :2 * heads * D].double().reshape(B, T, 2 * heads, D).split(D // 2, -1)
    return torch.cat([a * cos - b * sin, b * cos + a * sin], -1).reshape(B, T, 2 * heads * D)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("heads", [1, 5])
@pytest.mark.parametrize("T", [64, 192])
def test_rope_d128_matches_fp64(cuda, T, heads, inplace):
    from distributed_compute_pytorch_amd.ops.rope import apply_rope_qkv, rope_table

    torch.manual_seed(0)
    C = heads * D
    table = rope_table(256, 10000.0, cuda, head_dim=D)
    src = (torch.randn(2, T, 3 * C, device=cuda) * 2).to(BF)
    qkv = src.clone()
    y = apply_rope_qkv(qkv, heads, table, inplace=inplace)
    assert (y.data_ptr() == qkv.data_ptr()) == inplace
    assert _within_one_bf16_ulp(y[..., :2 * C], _rope64(src, heads, table))
    assert torch.equal(y[..., 2 * C:], src[..., 2 * C:])  # v: the input's bits
    g = torch.randn(2, T, 3 * C, device=cuda).to(BF)
    a = src.clone().requires_grad_()
    apply_rope_qkv(a * 1, heads, table, inplace=inplace).backward(g)
    assert _within_one_bf16_ulp(a.grad[..., :2 * C], _rope64(g, heads, table, sign=-1.0))
    assert torch.equal(a.grad[..., 2 * C:], g[..., 2 * C:])


def test_llama_d128_fused_matches_plain_fp32(cuda):
    """fused=True under bf16 autocast against the plain fp32 model; noise floor:
    the plain model's own bf16-autocast run (err < 4·noise + 2e-2)."""
    from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM
    from distributed_compute_pytorch_amd.ops.attention import attn_supported

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab=512, n_layer=2, n_head=2, n_embd=256, ffn_hidden=256, block_size=128)
    assert attn_supported(torch.empty(2, 128, 768, device=cuda, dtype=BF)[..., :256], 2, head_dim=128)
    fused = LlamaForCausalLM(cfg, fused=True).to(cuda)
    plain = LlamaForCausalLM(cfg, fused=False).to(cuda)
    plain.load_state_dict(fused.state_dict())
    idx = torch.randint(0, 512, (2, 128), device=cuda)
    tgt = idx.roll(-1, 1)

    def run(m, amp):
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF, enabled=amp):
            loss = m(idx, tgt)
        loss.backward()
        return float(loss.detach()), {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}

    l_ref, g_ref = run(plain, False)
    l_noise, g_noise = run(plain, True)
    l_fused, g_fused = run(fused, True)
    assert abs(l_fused - l_ref) < 4 * abs(l_noise - l_ref) + 2e-2 * max(1.0, abs(l_ref)), (l_fused, l_noise, l_ref)
    assert set(g_fused) == set(g_ref)
    for n, r in g_ref.items():
        den = float(r.norm().clamp_min(1e-3))
        err, noise = float((g_fused[n] - r).norm()) / den, float((g_noise[n] - r).norm()) / den
        print(f"{n}: fused err {err:.3e} plain-bf16 noise {noise:.3e}")
        assert err < 4 * noise + 2e-2, (n, err, noise)
