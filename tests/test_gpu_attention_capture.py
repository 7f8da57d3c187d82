"""The attention dropout under HIP-graph capture: the forward's device-resident
seed offset (``seed_offset=``; hash on seed + offset·0x9E3779B97F4A7C15) against
the integer oracle ``dropout_keep_mask(..., offset=)``, and the dropout counter
feeding it inside a capture, so that every replay draws a fresh keep mask whose
stored bits the backward follows."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 1234567891234
OFFSETS = (0, 1, 2**40 + 3)
CASES = [  # B, H, T, causal, p
    (1, 2, 128, False, 0.1),   # one query tile, two key blocks
    (1, 2, 192, True, 0.3),    # ragged tile, causal
    (1, 2, 128, False, 0.7),   # keep threshold >= 128 (the other SWAR compare)
]


def _qkv(B, H, T, cuda, seed, n=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, T, H * 64, generator=g).to(cuda).to(torch.bfloat16) for _ in range(n)]


def _off(k, cuda):
    return torch.tensor([k], dtype=torch.int64, device=cuda)


def _counter(cuda):
    from distributed_compute_pytorch_amd.ops import dropout

    dropout._ensure_counter(cuda)
    return dropout._COUNTER[cuda.index]


def _capture(fn, batched):
    """fn captured in a HIP graph (inside batched_offsets or plainly) after one
    eager warm-up on the capture stream; returns (graph, fn's captured result)."""
    from distributed_compute_pytorch_amd.ops.dropout import batched_offsets

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        with (batched_offsets() if batched else contextlib.nullcontext()):
            out = fn()
    return g, out


@pytest.mark.parametrize("case", CASES)
def test_seed_offset_matches_oracle(cuda, case):
    from distributed_compute_pytorch_amd.ops.attention import dropout_keep_mask, flash_attn_keep_bits

    B, H, T, causal, p = case
    q, k, v = _qkv(B, H, T, cuda, 11)
    tril = torch.ones(T, T, dtype=torch.bool, device=cuda).tril()
    seen = []
    for off in OFFSETS:
        got = flash_attn_keep_bits(q, k, v, H, causal, p, SEED, seed_offset=_off(off, cuda))
        want = dropout_keep_mask(B, H, T, p, SEED, cuda, offset=off)
        if causal:
            want = want & tril
        assert torch.equal(got, want), (off, int((got != want).sum()))
        seen.append(got)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


@pytest.mark.parametrize("case", CASES)
def test_zero_or_no_offset_is_bit_identical(cuda, case):
    from distributed_compute_pytorch_amd._ext import C as _C

    B, H, T, causal, p = case
    q, k, v = _qkv(B, H, T, cuda, 12)
    # the keep words the forward writes, [B*H][T/64][2][T]: causal, a wave (32
    # consecutive queries) skips the key blocks that begin after its last query;
    # their words stay unwritten memory
    nblk = T // 64
    written = torch.ones(nblk, T, dtype=torch.bool, device=cuda)
    if causal:
        last = torch.arange(T, device=cuda) | 31
        written = 64 * torch.arange(nblk, device=cuda)[:, None] <= last[None, :]
    written = written[None, :, None, :].expand(B * H, nblk, 2, T)

    def outputs(**kw):
        o, lse, words = _C.flash_attn_fwd(q, k, v, H, causal, p, SEED, **kw)
        return o, lse, words.view(B * H, nblk, 2, T)[written]

    base = outputs()
    for kw in ({"seed_offset": None}, {"seed_offset": _off(0, cuda)}):
        for name, a, b in zip(("o", "lse", "keep words"), outputs(**kw), base):
            assert torch.equal(a, b), (kw, name)


def test_seed_offset_with_key_mask(cuda):
    """The key-mask variant of the dropout forward: the last 64 keys hidden (their
    block is not visited, its keep words are not written)."""
    from distributed_compute_pytorch_amd._ext import C as _C
    from distributed_compute_pytorch_amd.ops.attention import decode_keep_bits, dropout_keep_mask, pack_key_mask

    B, H, T, causal, p = CASES[0]
    q, k, v = _qkv(B, H, T, cuda, 13)
    vis = torch.ones(B, T, dtype=torch.bool, device=cuda)
    vis[:, T - 64:] = False
    km = pack_key_mask(vis)
    base = _C.flash_attn_fwd(q, k, v, H, causal, p, SEED, True, km)
    for off in OFFSETS:
        o, lse, words = _C.flash_attn_fwd(q, k, v, H, causal, p, SEED, True, km, seed_offset=_off(off, cuda))
        got = decode_keep_bits(words, B, H, T, causal)[..., :T - 64]
        want = dropout_keep_mask(B, H, T, p, SEED, cuda, offset=off)[..., :T - 64]
        assert torch.equal(got, want), (off, int((got != want).sum()))
        if off == 0:
            assert torch.equal(o, base[0]) and torch.equal(lse, base[1])
            assert torch.equal(decode_keep_bits(base[2], B, H, T, causal)[..., :T - 64], got)


@pytest.mark.parametrize("batched", [False, True])
def test_fresh_masks_per_replay_with_consistent_backward(cuda, batched, monkeypatch):
    """Captured flash_attn_qkv forward + backward with a pinned host seed: replay
    r uses the mask of the counter value read before it, in o and in dq/dk/dv
    (bounds and reference of test_gpu_attention.py)."""
    from test_gpu_attention import _reference, _rel

    from distributed_compute_pytorch_amd.ops import attention

    B, H, T, causal, p = 1, 2, 128, True, 0.1
    C = H * 64
    monkeypatch.setattr(attention, "_seed", lambda: SEED)
    q, k, v, do = _qkv(B, H, T, cuda, 14, n=4)
    a = torch.cat([q, k, v], dim=2).requires_grad_(True)

    def fn():
        a.grad = None
        o = attention.flash_attn_qkv(a, H, causal, p)
        words = o.grad_fn.saved_tensors[3]
        o.backward(do)
        return o, words

    g, (o, words) = _capture(fn, batched)
    counter = _counter(cuda)
    tril = torch.ones(T, T, dtype=torch.bool, device=cuda).tril()
    masks = []
    for _ in range(3):
        torch.cuda.synchronize()
        c = int(counter.item())
        g.replay()
        torch.cuda.synchronize()
        keep = attention.dropout_keep_mask(B, H, T, p, SEED, cuda, offset=c)
        got = attention.decode_keep_bits(words, B, H, T, causal)
        assert torch.equal(got, keep & tril), (c, int((got != (keep & tril)).sum()))
        qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
        ref = _reference(qr, kr, vr, H, causal, p, keep.float())
        ref.backward(do.float())
        assert _rel(o, ref) < 1e-2, (c, _rel(o, ref))
        for i, (name, r) in enumerate((("dq", qr.grad), ("dk", kr.grad), ("dv", vr.grad))):
            err = _rel(a.grad[..., i * C:(i + 1) * C], r)
            assert err < 2e-2, (c, name, err)
        masks.append(got.clone())
    assert not torch.equal(masks[0], masks[1])
    assert not torch.equal(masks[1], masks[2])
    assert not torch.equal(masks[0], masks[2])


def test_two_calls_in_one_batched_replay(cuda):
    """Two attention calls and a Philox dropout inside batched_offsets: the two
    attention masks differ within a replay (own host seeds), both change from
    replay to replay, and the step-end add advances the counter by the same
    positive amount every time."""
    from distributed_compute_pytorch_amd.ops import attention, fused_dropout

    B, H, T, causal, p = 1, 2, 128, True, 0.1
    q, k, v, x = _qkv(B, H, T, cuda, 15, n=4)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, x)]

    def fn():
        for t in leaves:
            t.grad = None
        qa, ka, va, xa = leaves
        o1 = attention.flash_attn(qa, ka, va, H, causal, p)
        o2 = attention.flash_attn(qa, ka, va, H, causal, p)
        w1, w2 = o1.grad_fn.saved_tensors[5], o2.grad_fn.saved_tensors[5]
        (o1.float().sum() + o2.float().sum() + fused_dropout(xa, p).float().sum()).backward()
        return w1, w2

    g, (w1, w2) = _capture(fn, True)
    counter = _counter(cuda)
    torch.cuda.synchronize()
    values, masks = [int(counter.item())], []
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        values.append(int(counter.item()))
        m1, m2 = (attention.decode_keep_bits(w, B, H, T, causal) for w in (w1, w2))
        assert not torch.equal(m1, m2)
        masks.append((m1.clone(), m2.clone()))
    steps = [b - a for a, b in zip(values, values[1:])]
    assert steps[0] > 0 and steps == [steps[0]] * 3, values
    for i in range(2):
        for (a0, b0), (a1, b1) in ((masks[0], masks[1]), (masks[1], masks[2]), (masks[0], masks[2])):
            assert not torch.equal((a0, b0)[i], (a1, b1)[i])


def test_gpt2_attention_module_under_captured_step(cuda, monkeypatch):
    """models.gpt2's attention module under CapturedStep: in training mode two
    replays on one input differ (fresh attention dropout), in eval mode they
    are bit-identical."""
    from distributed_compute_pytorch_amd.models import gpt2
    from distributed_compute_pytorch_amd.utils.graphs import CapturedStep, capture_stream

    calls = []
    real = gpt2.flash_attn_qkv

    def spy(*args, **kw):
        calls.append(kw.get("dropout_p"))
        return real(*args, **kw)

    monkeypatch.setattr(gpt2, "flash_attn_qkv", spy)
    torch.manual_seed(0)
    cfg = gpt2.GPT2Config(vocab_size=512, n_positions=128, n_embd=128, n_layer=1, n_head=2, dropout=0.1)
    s = capture_stream()
    with torch.cuda.stream(s):
        attn = gpt2.CausalSelfAttention(cfg).to(cuda)
    x = torch.randn(1, 128, 128, generator=torch.Generator().manual_seed(16)).to(cuda)

    def step(inp):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return attn(inp)

    attn.train()
    cap = CapturedStep(step, [x.clone()], warmup=1, stream=s)
    assert calls and all(pd == 0.1 for pd in calls)  # the flash attention ran, with dropout
    y1 = cap(x).detach().clone()
    y2 = cap(x).detach().clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y1.float()).all())
    assert not torch.equal(y1, y2)

    attn.eval()
    del calls[:]
    cap = CapturedStep(step, [x.clone()], warmup=1, stream=s)
    assert calls and all(pd == 0.0 for pd in calls)
    z1 = cap(x).detach().clone()
    z2 = cap(x).detach().clone()
    torch.cuda.synchronize()
    assert torch.equal(z1, z2)


def test_attention_only_warmup_permits_capture(cuda, monkeypatch):
    """An eager attention call with dropout creates the device counter: a capture
    whose only earlier dropout was attention does not ask for a warm-up."""
    from distributed_compute_pytorch_amd.ops import attention, dropout

    monkeypatch.setattr(dropout, "_COUNTER", {})
    B, H, T = 1, 2, 128
    q, k, v = _qkv(B, H, T, cuda, 17)
    with torch.no_grad():
        g, o = _capture(lambda: attention.flash_attn(q, k, v, H, True, 0.1), False)
        g.replay()
        torch.cuda.synchronize()
    assert cuda.index in dropout._COUNTER and int(dropout._COUNTER[cuda.index].item()) == 1
    assert bool(torch.isfinite(o.float()).all())
