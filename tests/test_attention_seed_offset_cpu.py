"""The seed offset of the attention dropout, as far as it runs without a GPU:
``dropout_keep_mask(..., offset=k)`` hashes with seed + k·0x9E3779B97F4A7C15
(mod 2^64), and ``seed_offset=`` is validated before any native call."""
import pytest
import torch

GOLDEN64 = 0x9E3779B97F4A7C15
B, H, T, P = 1, 2, 256, 0.1
SEED = 1234567891234
OFFSETS = (1, 2, 1000)


@pytest.fixture(scope="module")
def masks():
    from distributed_compute_pytorch_amd.ops.attention import dropout_keep_mask

    return {k: dropout_keep_mask(B, H, T, P, SEED, offset=k) for k in OFFSETS}


def test_offset_zero_is_no_offset():
    from distributed_compute_pytorch_amd.ops.attention import dropout_keep_mask

    assert torch.equal(dropout_keep_mask(B, H, T, P, SEED, offset=0), dropout_keep_mask(B, H, T, P, SEED))


@pytest.mark.parametrize("k", OFFSETS + (2**40 + 3, 2**63 - 1))
def test_offset_is_a_seed_shift(k, masks):
    from distributed_compute_pytorch_amd.ops.attention import dropout_keep_mask

    got = masks[k] if k in masks else dropout_keep_mask(B, H, T, P, SEED, offset=k)
    want = dropout_keep_mask(B, H, T, P, (SEED + k * GOLDEN64) % 2**64)
    assert torch.equal(got, want)


def test_keep_rate_and_distinct_masks(masks):
    from distributed_compute_pytorch_amd.ops.attention import dropout_p_effective

    for k in OFFSETS:
        rate = float(masks[k].float().mean())
        assert abs(rate - (1 - dropout_p_effective(P))) < 0.01, (k, rate)
    for i, a in enumerate(OFFSETS):
        for b in OFFSETS[i + 1:]:
            assert not torch.equal(masks[a], masks[b]), (a, b)


@pytest.mark.parametrize("bad, exc", [(torch.zeros(1, dtype=torch.float32), TypeError),
                                      (torch.zeros(2, dtype=torch.int64), ValueError)])
def test_bad_seed_offset_is_rejected_before_the_native_call(bad, exc, monkeypatch):
    from distributed_compute_pytorch_amd.ops import attention

    class NoNative:
        def __getattr__(self, name):
            raise AssertionError(f"_C.{name} reached with an invalid seed_offset")

    monkeypatch.setattr(attention, "_C", NoNative())
    q = torch.zeros(1, 64, 64, dtype=torch.bfloat16)
    qkv = torch.zeros(1, 64, 192, dtype=torch.bfloat16)
    with pytest.raises(exc, match="seed_offset"):
        attention.flash_attn(q, q, q, 1, False, 0.1, seed_offset=bad)
    with pytest.raises(exc, match="seed_offset"):
        attention.flash_attn_qkv(qkv, 1, False, 0.1, seed_offset=bad)
    with pytest.raises(exc, match="seed_offset"):
        attention.flash_attn_keep_bits(q, q, q, 1, False, 0.1, 7, seed_offset=bad)
