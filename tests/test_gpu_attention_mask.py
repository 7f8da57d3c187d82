"""Key-padding masks in the MFMA flash attention (csrc/kernels/attention.hip,
KMASK instantiations) vs an fp32 PyTorch oracle of the same op: scores in
fp32, masked_fill(-inf) for hidden keys (and the causal triangle), softmax with
nan_to_num(0) (a row without a visible key is 0), the kernels' own dropout
keep-mask (``dropout_keep_mask``), · V — the construction and the tolerances of
``test_gpu_attention.py::_reference``. The K rows of hidden keys are scaled by
50: a kernel that takes the row max before masking fails visibly."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 1234567891234


def _lengths(T, lens):
    return torch.arange(T)[None, :] < torch.tensor(lens)[:, None]


def _mask_nonprefix():
    m = torch.rand(2, 192, generator=torch.Generator().manual_seed(11)) < 0.5
    m[0, 64:128] = False  # an interior empty block between two partly visible ones
    m[1, 0:64] = False    # the first block empty: the m = -inf start
    return m


def _mask_causal_pad():
    m = torch.ones(2, 256, dtype=torch.bool)
    m[0, :10] = False     # left padding: queries 0-9 see nothing
    m[1, 130:] = False    # a partly visible block that is a diagonal block of query tile 1
    return m


CASES = [  # B, H, T, causal, p, mask (CPU bool [B, T])
    (2, 2, 128, False, 0.0, lambda: _lengths(128, [128, 70])),
    (3, 2, 192, False, 0.1, lambda: _lengths(192, [64, 1, 191])),
    (2, 2, 192, False, 0.0, _mask_nonprefix),
    (2, 2, 256, True, 0.1, _mask_causal_pad),
    (2, 2, 128, False, 0.6, lambda: _lengths(128, [128, 0])),
    (1, 2, 256, True, 0.0, lambda: _lengths(256, [200])),
]


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12))


def _inputs(B, H, T, mask, dev, gen_seed=7):
    """Seeded randn bf16 q, k, v, do; the K rows of hidden keys times 50."""
    C = H * 64
    g = torch.Generator().manual_seed(gen_seed)
    q, k, v, do = (torch.randn(B, T, C, generator=g).to(dev).to(torch.bfloat16) for _ in range(4))
    if mask is not None:
        k = (k.float() * torch.where(mask.to(dev), 1.0, 50.0)[:, :, None]).to(torch.bfloat16)
    return q, k, v, do


def _run(q, k, v, do, H, causal, p, key_mask):
    from distributed_compute_pytorch_amd.ops.attention import flash_attn

    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    o = flash_attn(qa, ka, va, H, causal, p, SEED, key_mask=key_mask)
    dq, dk, dv = torch.autograd.grad(o, (qa, ka, va), do)
    return o.detach(), dq, dk, dv


def _reference(q, k, v, H, causal, p, keep, mask):
    from distributed_compute_pytorch_amd.ops.attention import dropout_p_effective

    B, T, C = q.shape

    def heads(t):
        return t.float().view(B, T, H, 64).transpose(1, 2)

    s = heads(q) @ heads(k).transpose(-1, -2) * 0.125
    hide = ~mask[:, None, None, :]
    if causal:
        hide = hide | torch.ones(T, T, dtype=torch.bool, device=q.device).triu(1)
    s = s.masked_fill(hide, float("-inf"))
    P = torch.softmax(s, -1).nan_to_num(0.0)
    if p > 0:
        P = P * keep / (1 - dropout_p_effective(p))
    return (P @ heads(v)).transpose(1, 2).reshape(B, T, C)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Kernel results and the oracle's for CASES[i], computed once."""
    from distributed_compute_pytorch_amd.ops.attention import dropout_keep_mask

    B, H, T, causal, p, mk = CASES[i]
    dev = torch.device("cuda", 0)
    mask = mk().to(dev)
    q, k, v, do = _inputs(B, H, T, mask, dev)
    got = _run(q, k, v, do, H, causal, p, mask)
    keep = dropout_keep_mask(B, H, T, p, SEED, dev).float() if p > 0 else None
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    ref = _reference(qr, kr, vr, H, causal, p, keep, mask)
    ref.backward(do.float())
    return mask, got, (ref.detach(), qr.grad, kr.grad, vr.grad)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_masked_flash_attn_matches_reference(cuda, i):
    B, H, T, causal, p, _ = CASES[i]
    mask, got, want = _case(i)
    names = ("o", "dq", "dk", "dv")
    for n, a in zip(names, got):
        assert a.shape == (B, T, H * 64) and a.dtype == torch.bfloat16
        assert bool(torch.isfinite(a).all()), n
    rels = {n: _rel(a, r) for n, a, r in zip(names, got, want)}
    print(CASES[i][:5], rels)
    assert rels["o"] < 1e-2, rels
    for n in ("dq", "dk", "dv"):
        assert rels[n] < 2e-2, (n, rels)
    o, dq, dk, dv = got
    # hidden keys: dk and dv rows exactly 0
    hidden = ~mask
    assert int(hidden.sum()) > 0
    assert not bool(dk[hidden].any()) and not bool(dv[hidden].any())
    # queries with no visible key (no key at all, or none at or before them under the causal mask)
    seen = (mask.cumsum(1) > 0) if causal else mask.any(1, keepdim=True).expand(B, T)
    blind = ~seen
    assert not bool(o[blind].any()) and not bool(dq[blind].any())
    if i in (3, 4):
        assert int(blind.sum()) > 0


@pytest.mark.parametrize("case", [(2, 3, 192, False, 0.1), (2, 2, 256, True, 0.1)])
def test_all_true_mask_is_bitwise_the_unmasked_call(cuda, case):
    """The masked kernels on an all-True mask compute exactly what the unmasked
    ones do (no atomics anywhere: bitwise)."""
    B, H, T, causal, p = case
    q, k, v, do = _inputs(B, H, T, None, cuda)
    plain = _run(q, k, v, do, H, causal, p, None)
    masked = _run(q, k, v, do, H, causal, p, torch.ones(B, T, dtype=torch.bool, device=cuda))
    for n, a, b in zip(("o", "dq", "dk", "dv"), masked, plain):
        assert torch.equal(a, b), n


def test_flash_attn_qkv_packed_with_mask(cuda):
    from distributed_compute_pytorch_amd.ops.attention import flash_attn, flash_attn_qkv

    B, H, T = 2, 4, 256
    C = H * 64
    g = torch.Generator().manual_seed(8)
    qkv = torch.randn(B, T, 3 * C, generator=g).to(cuda).to(torch.bfloat16)
    do = torch.randn(B, T, C, generator=g).to(cuda).to(torch.bfloat16)
    mask = _lengths(T, [256, 100]).to(cuda)
    a = qkv.clone().requires_grad_(True)
    o = flash_attn_qkv(a, H, True, 0.1, 42, key_mask=mask)
    o.backward(do)
    parts = [qkv[..., i * C:(i + 1) * C].contiguous().requires_grad_(True) for i in range(3)]
    o2 = flash_attn(*parts, H, True, 0.1, 42, key_mask=mask)
    o2.backward(do)
    assert torch.equal(o, o2)
    assert torch.equal(a.grad, torch.cat([t.grad for t in parts], dim=2))
    assert not bool(a.grad[1, 100:, C:].any())  # dk, dv of the hidden keys


def test_pack_key_mask_gpu_matches_cpu(cuda):
    """The HIP packer against the torch-ops implementation (bitwise), for the
    masks of the cases above, bool and 0/1 integer input; the packed tensor
    and the bool mask give equal results."""
    from distributed_compute_pytorch_amd.ops.attention import pack_key_mask

    for B, H, T, causal, p, mk in CASES:
        m = mk()
        want = pack_key_mask(m)
        assert want.shape == (B, 1 + T // 64) and want.dtype == torch.int64
        got = pack_key_mask(m.to(cuda))
        assert got.is_cuda and torch.equal(got.cpu(), want)
        assert torch.equal(pack_key_mask(m.to(cuda).to(torch.int32)).cpu(), want)
    B, H, T, causal, p, mk = CASES[1]
    m = mk().to(cuda)
    q, k, v, do = _inputs(B, H, T, m, cuda)
    for a, b in zip(_run(q, k, v, do, H, causal, p, m), _run(q, k, v, do, H, causal, p, pack_key_mask(m))):
        assert torch.equal(a, b)


def test_key_mask_graphs_capture(cuda):
    """What a captured masked forward + backward re-reads on replay (the
    flash_attn docstring): given the bool mask, the packer is inside the graph,
    so a replay equals the eager call bitwise and follows in-place changes of
    the mask's contents; given a tensor packed outside the capture, replays
    keep reading those packed bits and do not see such changes."""
    from distributed_compute_pytorch_amd.ops.attention import flash_attn, pack_key_mask

    B, H, T, causal, p = 2, 2, 256, False, 0.1
    m1 = _lengths(T, [256, 90]).to(cuda)
    m2 = _lengths(T, [130, 256]).to(cuda)
    q, k, v, do = _inputs(B, H, T, None, cuda)
    eager1 = _run(q, k, v, do, H, causal, p, m1)
    eager2 = _run(q, k, v, do, H, causal, p, m2)
    assert not torch.equal(eager1[0], eager2[0])

    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    mask = m1.clone()
    packed = pack_key_mask(mask)  # outside the capture

    def step(km):
        o = flash_attn(qa, ka, va, H, causal, p, SEED, key_mask=km)
        return (o,) + torch.autograd.grad(o, (qa, ka, va), do)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(mask)
    torch.cuda.current_stream().wait_stream(s)
    g_bool, g_packed = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_bool, stream=s):
        out_bool = step(mask)
    with torch.cuda.graph(g_packed, stream=s):
        out_packed = step(packed)

    def same(outs, want):
        torch.cuda.synchronize()
        return all(torch.equal(a.detach(), b) for a, b in zip(outs, want))

    g_bool.replay()
    g_packed.replay()
    assert same(out_bool, eager1) and same(out_packed, eager1)
    mask.copy_(m2)  # in place: the captured packer re-reads it
    g_bool.replay()
    g_packed.replay()
    assert same(out_bool, eager2)
    assert same(out_packed, eager1)  # packed before the capture: the change is not seen
    mask.copy_(m1)
    g_bool.replay()
    assert same(out_bool, eager1)
