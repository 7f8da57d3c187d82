"""fp8 Linear off the GPU: the row-quantisation recipe (``quantize_rows_reference``,
the GPU tests' oracle) and the fall-backs of ``Fp8Linear`` / ``LlamaConfig(fp8=True)``."""
import pytest
import torch
from torch import nn

from distributed_compute_pytorch_amd.models.llama import LlamaConfig, LlamaForCausalLM
from distributed_compute_pytorch_amd.ops.fp8 import Fp8Linear, quantize_rows_reference
from distributed_compute_pytorch_amd.ops.linear import FusedLinear

# format -> (mantissa bits m, half the smallest subnormal h, largest finite value)
FORMATS = {"e4m3": (3, 2.0 ** -10, 448.0), "e5m2": (2, 2.0 ** -17, 57344.0)}


def edge_rows(R, K, seed=0):
    """bf16 [R, K] of N(0, 1) rows holding zeros and bf16 subnormals; row 0 (and
    every 16th) all zero, row 1 (and every 16th) with one huge value."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, K, generator=g)
    x[:, 0::7] = 0.0
    x[:, 3::11] = 1e-39  # a bf16 subnormal
    x[0::16] = 0.0
    x[1::16, K // 2] = -3e38
    return x.to(torch.bfloat16)


def check_quantised(x, q, s, fmt):
    """The recipe's properties of (q, s) against the input x, in fp64."""
    m, h, fmax = FORMATS[fmt]
    x, q, s = x.double().cpu(), q.float().double().cpu(), s.double().cpu()
    assert not q.isnan().any() and not s.isnan().any() and bool((s > 0).all())
    assert float(q.abs().max()) <= fmax
    amax = x.abs().amax(1)
    assert bool((s * fmax >= amax * (1 - 2.0 ** -22)).all())
    zero = amax == 0
    assert bool((s[zero] == 1).all()) and bool((q[zero] == 0).all())
    err = (q * s[:, None] - x).abs()
    assert bool((err <= 2.0 ** -(m + 1) * x.abs() + s[:, None] * h).all())


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_reference_round_trip(fmt):
    x = edge_rows(40, 64)
    q, s = quantize_rows_reference(x, fmt)
    assert q.dtype == (torch.float8_e4m3fn if fmt == "e4m3" else torch.float8_e5m2) and s.dtype == torch.float32
    check_quantised(x, q, s, fmt)


@pytest.mark.parametrize("bias", [True, False])
def test_fp8_linear_module_on_cpu(bias):
    torch.manual_seed(0)
    ref = nn.Linear(128, 256, bias=bias)
    lin = Fp8Linear(128, 256, bias=bias)
    lin.load_state_dict(FusedLinear(128, 256, bias=bias).state_dict())  # same keys
    lin.load_state_dict(ref.state_dict())
    x = torch.randn(5, 128)
    assert torch.equal(lin(x), ref(x))


def test_llama_fp8_flag_on_cpu():
    cfg = dict(vocab=96, n_layer=2, n_head=2, n_embd=128, ffn_hidden=256, block_size=32)
    torch.manual_seed(0)
    a = LlamaForCausalLM(LlamaConfig(**cfg))
    b = LlamaForCausalLM(LlamaConfig(fp8=True, **cfg))
    b.load_state_dict(a.state_dict())
    assert isinstance(b.layers[0].attention.wo, Fp8Linear) and isinstance(b.layers[1].feed_forward.w2, Fp8Linear)
    assert not isinstance(b.layers[0].attention.wq, Fp8Linear) and not isinstance(a.layers[0].attention.wo, Fp8Linear)
    idx = torch.randint(0, 96, (2, 16))
    assert torch.equal(a(idx), b(idx))
