"""_C.fused_sgd / fused_adam / fused_adadelta / sumsq on CPU tensors vs the
fp64 one-step oracle of tests/multi_tensor_ref.py. The CPU loops of ops.cpp
carry the same expressions as the kernels, so this validates the oracle, the
bound and the tensor list without a GPU; the host checks (one dtype per call)
run before the device split and are tested here only."""
import pytest
import torch

import multi_tensor_ref as mt

CPU = torch.device("cpu")
CASES = [("sgd", "momentum_first_step"), ("sgd", "dampening_maximize_scaled"), ("adam", "default"),
         ("adam", "amsgrad_decoupled_wd"), ("adam", "maximize_scaled_betas"), ("adam", "fresh_state"),
         ("adadelta", "wd_maximize_scaled_rho")]


@pytest.fixture(scope="module")
def C():
    from distributed_compute_pytorch_amd._ext import C

    return C


def test_bound_tells_rounding_from_truncation():
    """The oracle's own teeth: round-to-nearest of the exact value passes with
    slack 0, truncation (error up to 1 ulp) does not, in every dtype."""
    g = torch.Generator().manual_seed(0)
    exact = (torch.rand(4096, generator=g, dtype=torch.float64) + 0.5) * torch.tensor([1.0, -1.0]).repeat(2048)
    for dtype in (mt.F32, mt.BF16, mt.F16):
        if dtype != mt.F32:  # fp32 values: torch converts fp64 to 16 bits through fp32, which rounds twice
            exact = exact.float().double()
        rne = exact.to(dtype)
        mt.assert_within(rne, exact, 0.0)
        shift = {mt.BF16: 16, mt.F16: 13, mt.F32: 29}[dtype]
        if dtype == mt.F32:
            trunc = ((exact.view(torch.int64) >> shift) << shift).view(torch.float64).float()
        else:
            trunc = ((exact.float().view(torch.int32) >> shift) << shift).view(torch.float32).to(dtype)
        with pytest.raises(AssertionError, match="outside the bound"):
            mt.assert_within(trunc, exact, 0.0)
    assert float(mt.ulp_dtype(torch.tensor([1.0, 1.5, 2.0, 0.0, 2.0 ** -20], dtype=torch.float64), mt.F16)[4]) \
        == 2.0 ** -24
    u = mt.ulp_dtype(torch.tensor([1.0, 1.99, 2.0, 0.0], dtype=torch.float64), mt.BF16)
    assert u.tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133]


def test_tensor_list_is_as_documented():
    xs = mt.ragged(CPU, mt.BF16, 0)
    numels = sorted(t.numel() for t in xs if t._base is None and t.dim() == 1 and t.numel())
    assert numels == [1, 2, 3, 4, 5, 7, 8191, 8192, 8193, 2 * 8192 + 2, 3 * 8192 + 1]
    assert xs[mt.EMPTY].numel() == 0 and 0 < mt.EMPTY < len(xs) - 1
    assert sum(t.is_contiguous(memory_format=torch.channels_last) and t.dim() == 4 for t in xs) == 1
    views = [t for t in xs if t._base is not None and t.dim() == 1 and t.numel()]
    assert [t.storage_offset() - mt.PAD for t in views] == [1, 2, 3]
    pads = mt.paddings(xs)
    assert len(pads) == 3 and all(int((p != mt.SENTINEL[mt.BF16]).sum()) == 0 and p.numel() >= 2 * mt.PAD for p in pads)
    assert max(t.numel() for t in xs) < 25000 and sum(t.numel() for t in xs) < 100000


@pytest.mark.parametrize("dtype", [mt.F32, mt.BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,case", CASES)
def test_one_step_oracle(C, kind, case, dtype):
    """Every output list of three synchronised steps within ulp_bound.
    adam/fresh_state is the case that fails when exp_avg_sq is scaled by
    1.f - float(beta2) instead of float(1 - beta2) (1.3e-5 against a slack of
    6.7e-7; NOTES §42)."""
    worst = mt.run_case(C, kind, case, CPU, dtype)
    print(f"worst relative error beyond the storage rounding, {kind}/{case}: {worst}")


@pytest.mark.parametrize("lo,hi", mt.RANGES)
def test_range_update_with_shadow(C, lo, hi):
    mt.run_range(C, CPU, lo, hi)


def test_sumsq_flag_tests_elements_not_the_sum(C):
    mt.check_sumsq_flags(C, CPU)


def test_one_dtype_per_call(C):
    """A gradient, state tensor or second parameter of another dtype would be
    read at the wrong element size: refused before any launch."""
    f = lambda n: torch.ones(n)  # noqa: E731
    h = lambda n: torch.ones(n, dtype=torch.bfloat16)  # noqa: E731
    msg = "one dtype per call"
    with pytest.raises(RuntimeError, match=msg):  # bf16 gradient, fp32 parameters
        C.fused_sgd([f(8)], [h(8)], [f(8)], 0.1, 0.9, 0.0, 0.0, False, False, False, 1.0)
    with pytest.raises(RuntimeError, match=msg):
        C.fused_adam([f(8)], [h(8)], [f(8)], [f(8)], [], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, False, False, False, 1.0)
    with pytest.raises(RuntimeError, match=msg):
        C.fused_adadelta([f(8)], [h(8)], [f(8)], [f(8)], 1.0, 0.9, 1e-6, 0.0, False, 1.0)
    with pytest.raises(RuntimeError, match=msg):  # fp32 state, bf16 parameters
        C.fused_sgd([h(8)], [h(8)], [f(8)], 0.1, 0.9, 0.0, 0.0, False, False, False, 1.0)
    with pytest.raises(RuntimeError, match=msg):
        C.fused_adam([h(8)], [h(8)], [h(8)], [f(8)], [], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, False, False, False, 1.0)
    with pytest.raises(RuntimeError, match=msg):
        C.fused_adam([h(8)], [h(8)], [h(8)], [h(8)], [f(8)], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, True, False, False, 1.0)
    with pytest.raises(RuntimeError, match=msg):
        C.fused_adadelta([h(8)], [h(8)], [h(8)], [f(8)], 1.0, 0.9, 1e-6, 0.0, False, 1.0)
    with pytest.raises(RuntimeError, match=msg):  # two parameter dtypes in one list
        C.fused_sgd([f(8), h(8)], [f(8), h(8)], [], 0.1, 0.0, 0.0, 0.0, False, False, False, 1.0)
    with pytest.raises(RuntimeError, match=msg):
        C.fused_adam([f(8), h(8)], [f(8), h(8)], [f(8), h(8)], [f(8), h(8)], [], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0,
                     False, False, False, 1.0)
    with pytest.raises(RuntimeError, match=msg):
        C.fused_adadelta([f(8), h(8)], [f(8), h(8)], [f(8), h(8)], [f(8), h(8)], 1.0, 0.9, 1e-6, 0.0, False, 1.0)
    # the unused amsgrad list is not looked at
    C.fused_adam([f(8)], [f(8)], [f(8)], [f(8)], [], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, False, False, False, 1.0)
