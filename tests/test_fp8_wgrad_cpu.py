"""fp8 weight gradient off the GPU: the transposing column-quantisation recipe
(``quantize_cols_t_reference``, the GPU tests' oracle) and ``LlamaConfig(fp8_wgrad=True)``."""
import pytest
import torch
from test_fp8_cpu import check_quantised, edge_rows

from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM
from distributed_compute_pytorch_amd.ops.fp8 import quantize_cols_t_reference


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_cols_reference_round_trip(fmt):
    x = edge_rows(40, 64)
    q, s = quantize_cols_t_reference(x, fmt)
    assert q.dtype == (torch.float8_e4m3fn if fmt == "e4m3" else torch.float8_e5m2) and q.shape == (64, 128)
    assert s.dtype == torch.float32 and s.shape == (64,)
    check_quantised(x.t(), q[:, :40], s, fmt)
    assert not q.view(torch.uint8)[:, 40:].any()


def test_llama_fp8_wgrad_flag_on_cpu():
    cfg = dict(vocab=96, n_layer=2, n_head=2, n_embd=128, ffn_hidden=256, block_size=32)
    with pytest.raises(ValueError):
        LlamaConfig(fp8_wgrad=True, **cfg)
    torch.manual_seed(0)
    a = LlamaForCausalLM(LlamaConfig(**cfg))
    b = LlamaForCausalLM(LlamaConfig(fp8=True, fp8_wgrad=True, **cfg))
    b.load_state_dict(a.state_dict())
    assert b.layers[0].attention.wo.wgrad == "fp8" and b.layers[1].feed_forward.w2.wgrad == "fp8"
    idx = torch.randint(0, 96, (2, 16))
    assert torch.equal(a(idx), b(idx))
