"""The fused BERT with a padding mask: the flash attention path (mask packed
once per forward, passed to every layer) against the unfused model on
scaled_dot_product_attention — the set-up and the autocast tolerances of
``test_gpu_models.py::test_fused_matches_stock_eval``."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_fused_bert_attention_mask_takes_flash_path(cuda, monkeypatch):
    from distributed_compute_pytorch_amd import models
    from distributed_compute_pytorch_amd.models import bert as bert_mod

    calls = {"flash": 0, "flash_masked": 0, "pack": 0}
    real_flash, real_pack = bert_mod.flash_attn_qkv, bert_mod.pack_key_mask

    def spy_flash(*a, **kw):
        calls["flash"] += 1
        calls["flash_masked"] += kw.get("key_mask") is not None
        return real_flash(*a, **kw)

    def spy_pack(*a, **kw):
        calls["pack"] += 1
        return real_pack(*a, **kw)

    monkeypatch.setattr(bert_mod, "flash_attn_qkv", spy_flash)
    monkeypatch.setattr(bert_mod, "pack_key_mask", spy_pack)

    torch.manual_seed(0)
    layers = 2
    a = models.bert_base(layers=layers, fused=True).to(cuda).eval()
    b = models.bert_base(layers=layers, fused=False).to(cuda).eval()
    b.load_state_dict(a.state_dict())
    B, T = 2, 128
    lens = torch.tensor([128, 75], device=cuda)
    ids = torch.randint(0, 30522, (B, T), device=cuda)
    am = (torch.arange(T, device=cuda)[None, :] < lens[:, None]).to(torch.int64)
    # MLM positions inside the valid lengths
    pos = (torch.rand(B, 20, device=cuda) * lens[:, None]).long().clamp_max(lens[:, None] - 1)
    kw = dict(attention_mask=am, mlm_positions=pos, mlm_labels=torch.randint(0, 30522, (B, 20), device=cuda),
              nsp_labels=torch.tensor([0, 1], device=cuda))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        la = a(ids, **kw)
        assert calls == {"flash": layers, "flash_masked": layers, "pack": 1}, calls
        lb = b(ids, **kw)
    assert calls == {"flash": layers, "flash_masked": layers, "pack": 1}, calls  # the unfused model: neither
    torch.testing.assert_close(la.float(), lb.float(), rtol=2e-2, atol=2e-2)
    la.backward()
    lb.backward()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        if p.grad is None:
            continue
        # (attention key biases have ~zero true gradient: floor the denominator)
        rel = (p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-3)
        assert rel < 0.1, (n, float(rel))
