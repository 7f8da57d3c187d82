"""Shared by the LAMB / LARS tests: the tensor list, fp64 references written
with plain torch ops from the formulas (You et al. 2019 / 2017; there is no
torch LAMB or LARS to compare against), and the checks that run on either
device.

Tensor list: test_gpu_kernels.SHAPES (1- and 5-element tensors; (8193,)
crosses a chunk boundary and has a scalar tail) plus
 - (300, 8192): 300 chunks, more than the reduce workgroup's 256 threads,
 - an all-zero parameter (‖p‖ = 0 → ratio 1),
 - a numel() == 0 tensor in the middle (table index != list index),
 - a view at element offset 1 of a larger buffer (unaligned: scalar path),
and, in a weight_decay = 0 group, a parameter whose gradient is all zero
(‖u‖ = 0 → ratio 1, no NaN) and an ordinary one.
"""
import functools

import torch

from test_gpu_kernels import SHAPES

STEPS = 4
VIEW, ZERO_GRAD = 10, 11  # indices in the list below


def _values(seed):
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(s, generator=g) for s in SHAPES]
    vals.append(torch.randn(300, 8192, generator=g))
    vals.append(torch.zeros(257))
    vals.append(torch.zeros(0))
    vals.append(torch.randn(4099, generator=g))  # VIEW
    vals.append(torch.randn(513, generator=g))   # ZERO_GRAD
    vals.append(torch.randn(33, 65, generator=g))
    return vals


GROUP = [0] * (len(SHAPES) + 4) + [1, 1]  # 0: the weight-decay group, 1: weight_decay = 0


def make_params(dev, dtype, seed=0):
    """The tensor list on ``dev`` as leaf tensors (plain, not nn.Parameter, so
    the offset view stays a view)."""
    out = []
    for i, v in enumerate(_values(seed)):
        if i == VIEW:
            buf = torch.zeros(v.numel() + 16, device=dev, dtype=dtype)
            p = buf[1:1 + v.numel()]
            p.copy_(v)
            assert p.storage_offset() == 1
        else:
            p = v.to(dev, dtype)
        out.append(p)
    return out


def make_grads(dev, dtype, it):
    gs = [g.to(dev, dtype) for g in _values(1000 + it)]
    gs[ZERO_GRAD].zero_()
    gs[8] = torch.randn(257, generator=torch.Generator().manual_seed(2000 + it)).to(dev, dtype)
    return gs


def clone_params(ps):
    """Independent copies with the same layout (the view stays at offset 1)."""
    out = []
    for i, p in enumerate(ps):
        if i == VIEW:
            buf = torch.zeros(p.numel() + 16, device=p.device, dtype=p.dtype)
            q = buf[1:1 + p.numel()]
            q.copy_(p)
        else:
            q = p.detach().clone()
        out.append(q)
    return out


LAMB_DEFAULT = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, bias_correction=True,
                    always_adapt=False, max_grad_norm=0.0, maximize=False, grad_scale=1.0)
LAMB_CASES = {
    "default": {},
    "no_bias_correction": dict(bias_correction=False),
    "always_adapt": dict(always_adapt=True),
    "maximize_scaled": dict(maximize=True, grad_scale=0.25, betas=(0.8, 0.95)),
    "clipped": dict(max_grad_norm=1.0),
    "clipped_scaled_adapt": dict(max_grad_norm=50.0, grad_scale=0.5, always_adapt=True, bias_correction=False),
}
LARS_DEFAULT = dict(lr=0.5, momentum=0.9, dampening=0.0, weight_decay=1e-2, nesterov=False, trust_coefficient=0.02,
                    eps=1e-8, always_adapt=False, maximize=False, grad_scale=1.0)
LARS_CASES = {
    "default": {},
    "nesterov_adapt": dict(nesterov=True, always_adapt=True),
    "dampening_maximize": dict(dampening=0.3, maximize=True, grad_scale=0.25),
    "no_momentum": dict(momentum=0.0, always_adapt=True),
}


def lamb_cfg(name):
    return {**LAMB_DEFAULT, **LAMB_CASES[name]}


def lars_cfg(name):
    return {**LARS_DEFAULT, **LARS_CASES[name]}


def _wd(cfg, i):
    return cfg["weight_decay"] if GROUP[i] == 0 else 0.0


# ------------------------------------------------------------ fp64 references
def lamb_ref_step(p, g, m, v, step, cfg):
    """One LAMB step on fp64 lists, in place; returns the trust ratios."""
    b1, b2 = cfg["betas"]
    clip = 1.0
    if cfg["max_grad_norm"] > 0:
        norm = torch.sqrt(sum((x.double() * cfg["grad_scale"]).pow(2).sum() for x in g))
        clip = min(1.0, cfg["max_grad_norm"] / (float(norm) + 1e-6))
    bc1 = 1.0 - b1 ** step if cfg["bias_correction"] else 1.0
    bc2_sqrt = (1.0 - b2 ** step) ** 0.5 if cfg["bias_correction"] else 1.0
    ratios = []
    for i in range(len(p)):
        wd = _wd(cfg, i)
        gi = g[i].double() * (cfg["grad_scale"] * clip)
        if cfg["maximize"]:
            gi = -gi
        m[i].mul_(b1).add_(gi, alpha=1.0 - b1)
        v[i].mul_(b2).add_(gi * gi, alpha=1.0 - b2)
        u = (m[i] / bc1) / (v[i].sqrt() / bc2_sqrt + cfg["eps"]) + wd * p[i]
        pn, un = float(p[i].norm()), float(u.norm())
        adapts = wd != 0 or cfg["always_adapt"]
        r = pn / un if (adapts and pn > 0 and un > 0) else 1.0
        p[i].sub_(u, alpha=cfg["lr"] * r)
        ratios.append(r)
    return ratios


def lars_ref_step(p, g, buf, step, cfg):
    """One LARS step on fp64 lists, in place (buf[i] None before the first
    step); returns the local rates."""
    mom = cfg["momentum"]
    ratios = []
    for i in range(len(p)):
        wd = _wd(cfg, i)
        gi = g[i].double() * cfg["grad_scale"]
        if cfg["maximize"]:
            gi = -gi
        pn, gn = float(p[i].norm()), float(gi.norm())
        adapts = wd != 0 or cfg["always_adapt"]
        local = cfg["trust_coefficient"] * pn / (gn + wd * pn + cfg["eps"]) if (adapts and pn > 0 and gn > 0) else 1.0
        d = local * (gi + wd * p[i])
        if mom != 0:
            if buf[i] is None:
                buf[i] = d.clone()
            else:
                buf[i].mul_(mom).add_(d, alpha=1.0 - cfg["dampening"])
            d = d + mom * buf[i] if cfg["nesterov"] else buf[i]
        p[i].sub_(d, alpha=cfg["lr"])
        ratios.append(local)
    return ratios


@functools.lru_cache(maxsize=None)
def reference(kind, case, dtype, dev_str):
    """(parameters after each step, ratios of each step) of the fp64 reference
    from the ``dtype``-rounded start and gradients. Computed once per
    configuration; callers must not modify it."""
    dev = torch.device(dev_str)
    cfg = lamb_cfg(case) if kind == "lamb" else lars_cfg(case)
    p = [x.double() for x in make_params(dev, dtype)]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    buf = [None] * len(p)
    params, ratios = [], []
    for it in range(STEPS):
        g = make_grads(dev, dtype, it)
        if kind == "lamb":
            ratios.append(lamb_ref_step(p, g, m, v, it + 1, cfg))
        else:
            ratios.append(lars_ref_step(p, g, buf, it + 1, cfg))
        params.append([x.clone() for x in p])
    return params, ratios


def tolerances(dtype):
    """fp32: the project's bound for fused Adam vs torch. The only extra error
    is the ratio's: each thread adds at most 32 fp32 terms serially, then a
    fixed tree, so Σx² is within a few 2⁻²⁴·32 ≈ 2e-6 relative and the square
    root halves that. bf16: the project's bound for bf16 SGD."""
    return dict(rtol=1e-5, atol=1e-6) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)


# ------------------------------------------------------ runs of the project's
def groups_of(ps, cfg):
    g0 = [p for i, p in enumerate(ps) if GROUP[i] == 0]
    g1 = [p for i, p in enumerate(ps) if GROUP[i] == 1]
    return [{"params": g0}, {"params": g1, "weight_decay": 0.0}]


def make_optimizer(kind, ps, cfg, **extra):
    import distributed_compute_pytorch_amd as dcp

    kw = {k: v for k, v in cfg.items() if k != "grad_scale"}
    kw.update(extra)
    cls = dcp.optim.LAMB if kind == "lamb" else dcp.optim.LARS
    return cls(groups_of(ps, cfg), **kw)


def set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g


def check_optimizer(kind, case, dev, dtype):
    """dcp.optim.LAMB / LARS over STEPS steps vs the fp64 reference."""
    cfg = lamb_cfg(case) if kind == "lamb" else lars_cfg(case)
    ps = make_params(dev, dtype)
    opt = make_optimizer(kind, ps, cfg)
    for it in range(STEPS):
        set_grads(ps, make_grads(dev, dtype, it))
        opt.step(grad_scale=cfg["grad_scale"])
    ref, _ = reference(kind, case, dtype, str(dev))
    for i, (p, r) in enumerate(zip(ps, ref[-1])):
        assert bool(torch.isfinite(p.float()).all()), i
        torch.testing.assert_close(p.double(), r, msg=lambda s, i=i: f"tensor {i}: {s}", **tolerances(dtype))
    return opt, ps


def run_op(kind, case, dev, dtype, steps=STEPS, ps=None):
    """The same steps through _C.fused_lamb / _C.fused_lars directly (one call
    per group, state kept here). Returns (params, state lists, ratios per step
    in list order)."""
    from distributed_compute_pytorch_amd._ext import C

    cfg = lamb_cfg(case) if kind == "lamb" else lars_cfg(case)
    ps = make_params(dev, dtype) if ps is None else ps
    m = [torch.zeros_like(p) for p in ps]
    v = [torch.zeros_like(p) for p in ps]
    ratios = []
    for it in range(steps):
        gs = make_grads(dev, dtype, it)
        clip = None
        if kind == "lamb" and cfg["max_grad_norm"] > 0:
            norm = C.sumsq([g for g in gs if g.numel()])[0].sqrt() * cfg["grad_scale"]
            clip = torch.clamp(cfg["max_grad_norm"] / (norm + 1e-6), max=1.0).reshape(1).float()
        row = [None] * len(ps)
        for grp in (0, 1):
            idx = [i for i in range(len(ps)) if GROUP[i] == grp]
            sel = lambda l: [l[i] for i in idx]  # noqa: E731
            wd = cfg["weight_decay"] if grp == 0 else 0.0
            if kind == "lamb":
                b1, b2 = cfg["betas"]
                r = C.fused_lamb(sel(ps), sel(gs), sel(m), sel(v), cfg["lr"], b1, b2, cfg["eps"], wd, float(it + 1),
                                 cfg["bias_correction"], cfg["always_adapt"], cfg["maximize"], cfg["grad_scale"],
                                 clip)
            else:
                r = C.fused_lars(sel(ps), sel(gs), sel(m) if cfg["momentum"] != 0 else [], cfg["lr"],
                                 cfg["momentum"], cfg["dampening"], wd, cfg["nesterov"], cfg["maximize"], it == 0,
                                 cfg["trust_coefficient"], cfg["eps"], cfg["always_adapt"], cfg["grad_scale"])
            assert r.dtype == torch.float32 and r.device == ps[0].device and r.shape == (len(idx),)
            for k, i in enumerate(idx):
                row[i] = r[k]
        ratios.append(torch.stack(row))
    return ps, (m, v), ratios


def check_op_ratios(kind, case, dev, dtype):
    """Per-step ratios (and the parameters) of the op vs the fp64 reference.
    bf16: the first step's ratios see identical inputs and fp32 math, so they
    meet the fp32 bound; later ones inherit the bf16 rounding of the state."""
    ps, _, ratios = run_op(kind, case, dev, dtype)
    ref_p, ref_r = reference(kind, case, dtype, str(dev))
    for it in range(STEPS):
        want = torch.tensor(ref_r[it], dtype=torch.float64)
        tol = 1e-5 if (dtype == torch.float32 or it == 0) else 3e-2
        torch.testing.assert_close(ratios[it].double().cpu(), want, rtol=tol, atol=0.0,
                                   msg=lambda s, it=it: f"step {it}: {s}")
    n_empty = [i for i, p in enumerate(ps) if p.numel() == 0]
    assert n_empty and all(float(ratios[0][i]) == 1.0 for i in n_empty)
    for i, (p, r) in enumerate(zip(ps, ref_p[-1])):
        torch.testing.assert_close(p.double(), r, msg=lambda s, i=i: f"tensor {i}: {s}", **tolerances(dtype))
    return ratios
