"""CPU side of the key-padding mask: the torch-ops ``pack_key_mask`` (the HIP
packer's oracle) against a plain Python loop, and the fused BERT's fallback
with an ``attention_mask`` off the GPU."""
import torch


def _pack_loop(mask):
    B, T = mask.shape
    rows = []
    for b in range(B):
        words, count = [], 0
        for blk in range(T // 64):
            w = sum(1 << j for j in range(64) if mask[b, 64 * blk + j])
            if w:
                count = blk + 1
            words.append(w - (1 << 64) if w >= 1 << 63 else w)  # the 64-bit pattern as int64
        rows.append([count] + words)
    return torch.tensor(rows, dtype=torch.int64)


def test_pack_key_mask_cpu_matches_loop():
    from distributed_compute_pytorch_amd.ops.attention import pack_key_mask

    m = torch.rand(3, 192, generator=torch.Generator().manual_seed(3)) < 0.5
    got = pack_key_mask(m)
    assert got.dtype == torch.int64 and got.shape == (3, 4)
    assert torch.equal(got, _pack_loop(m))
    assert torch.equal(pack_key_mask(m.to(torch.int32)), got)  # 0/1 integers


def test_pack_key_mask_block_count():
    from distributed_compute_pytorch_amd.ops.attention import pack_key_mask

    m = torch.zeros(3, 192, dtype=torch.bool)
    m[1, :128] = True      # the last visible key is the last key of block 1
    m[2, 5] = True
    m[2, 191] = True       # bit 63 of the last block
    got = pack_key_mask(m)
    assert got[:, 0].tolist() == [0, 2, 3]
    assert got[0, 1:].tolist() == [0, 0, 0]
    assert got[1, 1:].tolist() == [-1, -1, 0]
    assert got[2, 1:].tolist() == [1 << 5, 0, -(1 << 63)]
    assert torch.equal(got, _pack_loop(m))


def test_fused_bert_cpu_attention_mask_falls_back():
    """Off the GPU the fused model keeps the SDPA path for a padding mask: it
    equals the unfused model."""
    from distributed_compute_pytorch_amd import models

    torch.manual_seed(0)
    kw = dict(layers=2, hidden=128, heads=2, intermediate=256, vocab_size=1000, max_position=64)
    a = models.bert_base(fused=True, **kw).eval()
    b = models.bert_base(fused=False, **kw).eval()
    b.load_state_dict(a.state_dict())
    ids = torch.randint(0, 1000, (2, 64))
    am = (torch.arange(64)[None, :] < torch.tensor([64, 40])[:, None]).to(torch.int64)
    pos = torch.randint(0, 40, (2, 5))
    args = dict(attention_mask=am, mlm_positions=pos, mlm_labels=torch.randint(0, 1000, (2, 5)),
                nsp_labels=torch.tensor([0, 1]))
    la, lb = a(ids, **args), b(ids, **args)
    torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-5)
    xa, _ = a(ids, attention_mask=am)
    xb, _ = b(ids, attention_mask=am)
    torch.testing.assert_close(xa, xb, rtol=1e-4, atol=1e-5)
