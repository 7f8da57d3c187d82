"""dcp.optim.LAMB / LARS on the CPU path of _C.fused_lamb / _C.fused_lars vs
fp64 references (tests/layerwise_ref.py), plus the properties that do not
need a GPU: checkpoint round trip, independence of the thread count, and the
DDP optimizer overlap on the host backend."""
import copy

import pytest
import torch
import torch.nn.functional as F

import layerwise_ref as lw
from mp_util import run_world

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", list(lw.LAMB_CASES))
def test_lamb_matches_fp64(case, dtype):
    opt, ps = lw.check_optimizer("lamb", case, CPU, dtype)
    st = opt.state[ps[0]]
    assert set(st.keys()) == {"step", "exp_avg", "exp_avg_sq"}
    assert float(st["step"]) == lw.STEPS and st["step"].dtype == torch.float32 and not st["step"].is_cuda
    assert st["exp_avg"].dtype == dtype and st["exp_avg_sq"].dtype == dtype


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", list(lw.LARS_CASES))
def test_lars_matches_fp64(case, dtype):
    opt, ps = lw.check_optimizer("lars", case, CPU, dtype)
    want = {"momentum_buffer"} if lw.lars_cfg(case)["momentum"] != 0 else set()
    assert set(opt.state[ps[0]].keys()) == want


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,case", [("lamb", "default"), ("lamb", "always_adapt"), ("lamb", "clipped_scaled_adapt"),
                                       ("lars", "default"), ("lars", "nesterov_adapt")])
def test_returned_ratios_match_fp64(kind, case, dtype):
    ratios = lw.check_op_ratios(kind, case, CPU, dtype)
    r0 = ratios[0]
    assert float(r0[8]) == 1.0  # the all-zero parameter: ‖p‖ = 0
    assert float(r0[lw.ZERO_GRAD]) == 1.0  # ‖u‖ = 0 (always_adapt) or a group that does not adapt
    adapts_plain = lw.lamb_cfg(case)["always_adapt"] if kind == "lamb" else lw.lars_cfg(case)["always_adapt"]
    assert (float(r0[-1]) != 1.0) == adapts_plain  # the ordinary tensor of the weight_decay = 0 group
    assert float(r0[2]) != 1.0


def test_optimizer_equals_op():
    """The optimizer adds nothing to the op's numbers: same bits."""
    for kind in ("lamb", "lars"):
        _, ps = lw.check_optimizer(kind, "default", CPU, torch.float32)
        qs, _, _ = lw.run_op(kind, "default", CPU, torch.float32)
        for p, q in zip(ps, qs):
            assert torch.equal(p, q)


@pytest.mark.parametrize("kind", ["lamb", "lars"])
def test_state_dict_round_trip_continues_bit_identically(kind):
    cfg = lw.lamb_cfg("always_adapt") if kind == "lamb" else lw.lars_cfg("dampening_maximize")
    ps = lw.make_params(CPU, torch.float32)
    opt = lw.make_optimizer(kind, ps, cfg)
    for it in range(2):
        lw.set_grads(ps, lw.make_grads(CPU, torch.float32, it))
        opt.step(grad_scale=cfg["grad_scale"])
    qs = lw.clone_params(ps)
    opt2 = lw.make_optimizer(kind, qs, cfg)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    for it in range(2, 4):
        for o, xs in ((opt, ps), (opt2, qs)):
            lw.set_grads(xs, lw.make_grads(CPU, torch.float32, it))
            o.step(grad_scale=cfg["grad_scale"])
    for p, q in zip(ps, qs):
        assert torch.equal(p, q)
    for p, q in zip(ps, qs):
        for k, a in opt.state[p].items():
            assert torch.equal(a, opt2.state[q][k]), k


def test_lamb_independent_of_thread_count():
    before = torch.get_num_threads()
    runs = []
    try:
        for n in (1, 4):
            torch.set_num_threads(n)
            ps, (m, v), ratios = lw.run_op("lamb", "always_adapt", CPU, torch.float32, steps=2)
            runs.append(ps + m + v + ratios)
    finally:
        torch.set_num_threads(before)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _overlap_lamb(rank, world):
    """LAMB under overlap_optimizer steps bucket by bucket on whole parameters
    (a per-tensor norm cannot be updated in ranges): bit-identical to the
    non-overlapped run, nothing left deferred."""
    import distributed_compute_pytorch_amd as dcp
    from distributed_compute_pytorch_amd.models import ConvNet

    torch.manual_seed(0)
    base = ConvNet()
    runs = {}
    for ov in (False, True):
        m = copy.deepcopy(base)
        ddp = dcp.parallel.DistributedDataParallel(m, gradient_as_bucket_view=True, bucket_cap_mb=0.05,
                                                   overlap_optimizer=ov)
        decay = [p for p in ddp.parameters() if p.ndim > 1]
        rest = [p for p in ddp.parameters() if p.ndim <= 1]
        opt = dcp.optim.LAMB([{"params": decay}, {"params": rest, "weight_decay": 0.0}], lr=1e-2)
        g = torch.Generator().manual_seed(7 + rank)
        deferred = []
        for it in range(4):
            opt.zero_grad(set_to_none=True)
            x, y = torch.randn(8, 1, 28, 28, generator=g), torch.randint(0, 10, (8,), generator=g)
            with torch.random.fork_rng():
                torch.manual_seed(it)
                F.nll_loss(ddp(x), y).backward()
            deferred.append(len(ddp.reducer.deferred_buckets()))
            opt.step()
            assert ddp.reducer.deferred_buckets() == []
        if ov:
            nb = len(ddp.bucket_sizes())
            assert deferred[0] == 0 and all(d == nb for d in deferred[1:]), (deferred, nb)
        else:
            assert deferred == [0] * 4
        runs[ov] = [p.detach().clone() for p in m.parameters()]
    for a, b in zip(runs[False], runs[True]):
        assert torch.equal(a, b)


def test_lamb_overlap_optimizer_matches():
    run_world(_overlap_lamb, 2)
