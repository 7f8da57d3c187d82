"""Shared by the multi-tensor kernel tests (SGD / Adam / Adadelta, mt_copy,
sumsq, scale_by): fp64 one-step references written with plain torch ops from
the formulas in the torch.optim documentation, the elementwise bound they are
compared with, the tensor list, and the case runners that work on either
device. Nothing here imports the package under test: the runners take the
extension module (``_C``) as an argument.

Bound. ``ulp_bound(exact, dtype, slack) = 0.5·ulp_dtype(exact) + slack·|exact|
+ TINY`` per element, asserted on every element. The first term is the one
rounding to the stored dtype; ``slack`` is the error of the fp32 registers
before that rounding. The slacks are not taken from the code under test: the
same step is evaluated in plain torch fp32 on the CPU (``model_*`` below), its
largest relative deviation from the fp64 result is measured per output over
these inputs (``python tests/multi_tensor_ref.py`` prints the table), and
SLACK holds 4× that, rounded up (the kernels' fmaf contractions and division
order differ from torch's by a few roundings). NOTES §42 has the figures.

Inputs. slack·|exact| is a relative bound, so the inputs keep every sum away
from cancellation: element i of the parameter, of the effective gradient
(negated under ``maximize``) and of the first-moment state share one random
sign s_i, and the magnitudes keep lr·update below |p|. Second-moment state is
positive. Both signs of every quantity still occur.
"""
import math

import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
DTYPE_IDS = ["fp32", "bf16", "fp16"]
CHUNK = 8192
TINY = 2.0 ** -1000

_MANT = {F32: 23, BF16: 7, F16: 10}
_EMIN = {F32: -126, BF16: -126, F16: -14}
_INT = {F32: torch.int32, BF16: torch.int16, F16: torch.int16}
SENTINEL = {F32: 0x7FC0DEAD, BF16: 0x7FD5, F16: 0x7DD5}  # NaNs with a payload

# 4 × the measured deviation of the fp32 model from fp64, rounded up (NOTES §42).
SLACK = {
    "sgd": {"p": 3.5e-7, "buf": 5.6e-7},
    "adam": {"p": 5.0e-7, "m": 5.6e-7, "v": 6.7e-7, "vmax": 5.2e-7},
    "adadelta": {"p": 2.8e-7, "sq": 5.7e-7, "acc": 5.7e-7},
    # bias corrections from powf(beta, step) in fp32 (capturable mode): only p sees them
    "adam_device_step": {"p": 2.3e-6, "m": 5.6e-7, "v": 6.7e-7, "vmax": 5.2e-7},
    # Σx²: fmaf chains of <= 32 terms, wave tree, serial over waves and chunks
    "sumsq": 3.6e-7,
    # scale · x with scale not a power of two: one fp32 multiply before the store
    "scale": 2.4e-7,
}


# ------------------------------------------------------------------ bound ---
def ulp_dtype(exact, dtype):
    """Spacing of ``dtype`` at |exact| (fp64 tensor): 2^(e - mantissa bits),
    the subnormal spacing below the smallest normal."""
    a = exact.detach().abs().double()
    _, ex = torch.frexp(a)  # a = f · 2^ex, f in [0.5, 1)
    e = torch.where(a > 0, ex - 1, torch.full_like(ex, _EMIN[dtype])).clamp(min=_EMIN[dtype])
    # 2^k built from its bit pattern: ldexp / pow are not exact on every device
    return ((e.to(torch.int64) - _MANT[dtype] + 1023) << 52).view(torch.float64)


def ulp_bound(exact, dtype, slack):
    return 0.5 * ulp_dtype(exact, dtype) + slack * exact.detach().abs().double() + TINY


def assert_within(got, exact, slack, what=""):
    """Every element of ``got`` (stored dtype) within ulp_bound of ``exact``
    (fp64). Returns the largest relative error in excess of the storage
    rounding, max((|got - exact| - 0.5 ulp) / |exact|): the figure to compare
    with the slack."""
    assert got.shape == exact.shape, what
    if got.numel() == 0:
        return 0.0
    g = got.detach().double()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite result"
    err = (g - exact).abs()
    half = 0.5 * ulp_dtype(exact, got.dtype)
    bound = half + slack * exact.abs() + TINY
    bad = err > bound
    if bool(bad.any()):
        k = int(torch.argmax((err / bound).flatten()))
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at flat index {k}: "
            f"got {float(g.flatten()[k])!r}, exact {float(exact.flatten()[k])!r}, "
            f"|err| {float(err.flatten()[k]):.3e} > bound {float(bound.flatten()[k]):.3e} "
            f"(0.5 ulp {float(half.flatten()[k]):.3e}, slack {slack:g})")
    return float(((err - half).clamp(min=0) / exact.abs().clamp(min=1e-300)).max())


def bits(t):
    """The tensor's bit patterns as integers (for bit-for-bit comparisons)."""
    return t.detach().view(_INT[t.dtype])


# ----------------------------------------------------- one-step references ---
def _sgd(p, g, buf, c):
    g = g * c["grad_scale"]
    if c["maximize"]:
        g = -g
    if c["weight_decay"] != 0:
        g = g + c["weight_decay"] * p
    b = None
    if c["momentum"] != 0:
        b = g.clone() if c["first_step"] else c["momentum"] * buf + c["omd"] * g
        g = g + c["momentum"] * b if c["nesterov"] else b
    return p - c["lr"] * g, b


def _adam(p, g, m, v, vmax, c, bc1, bc2_sqrt):
    g = g * c["grad_scale"]
    if c["maximize"]:
        g = -g
    if c["weight_decay"] != 0:
        if c["decoupled"]:
            p = p * (1.0 - c["lr"] * c["weight_decay"])
        else:
            g = g + c["weight_decay"] * p
    m = c["beta1"] * m + c["omb1"] * g
    v = c["beta2"] * v + c["omb2"] * (g * g)
    if c["amsgrad"]:
        vmax = torch.maximum(vmax, v)
        denom = vmax.sqrt() / bc2_sqrt + c["eps"]
    else:
        denom = v.sqrt() / bc2_sqrt + c["eps"]
    return p - (c["lr"] / bc1) * (m / denom), m, v, vmax


def _adadelta(p, g, sq, acc, c):
    g = g * c["grad_scale"]
    if c["maximize"]:
        g = -g
    if c["weight_decay"] != 0:
        g = g + c["weight_decay"] * p
    sq = c["rho"] * sq + c["omr"] * (g * g)
    delta = (acc + c["eps"]).sqrt() / (sq + c["eps"]).sqrt() * g
    acc = c["rho"] * acc + c["omr"] * (delta * delta)
    return p - c["lr"] * delta, sq, acc


SGD_DEFAULT = dict(lr=0.05, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False,
                   first_step=False, grad_scale=1.0)
ADAM_DEFAULT = dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, amsgrad=False,
                    maximize=False, grad_scale=1.0)
ADADELTA_DEFAULT = dict(lr=1.0, rho=0.9, eps=1e-6, weight_decay=0.0, maximize=False, grad_scale=1.0)


def _d(x):
    return None if x is None else x.detach().double()


def _f(x):
    return None if x is None else x.detach().float()


def ref_sgd_step(p, g, buf=None, **kw):
    """Exact (fp64) result of one torch.optim.SGD step from the stored tensors
    (any dtype): (p, momentum buffer or None)."""
    c = {**SGD_DEFAULT, **kw}
    c["omd"] = 1.0 - c["dampening"]
    return _sgd(_d(p), _d(g), _d(buf), c)


def ref_adam_step(p, g, m, v, vmax=None, *, step, **kw):
    """Exact result of one Adam / AdamW (``decoupled``) step at ``step``
    (1-based): (p, exp_avg, exp_avg_sq, max_exp_avg_sq or None)."""
    c = {**ADAM_DEFAULT, **kw}
    c["omb1"], c["omb2"] = 1.0 - c["beta1"], 1.0 - c["beta2"]
    bc1 = 1.0 - c["beta1"] ** step
    bc2_sqrt = math.sqrt(1.0 - c["beta2"] ** step)
    return _adam(_d(p), _d(g), _d(m), _d(v), _d(vmax), c, bc1, bc2_sqrt)


def ref_adadelta_step(p, g, sq, acc, **kw):
    """Exact result of one Adadelta step: (p, square_avg, acc_delta)."""
    c = {**ADADELTA_DEFAULT, **kw}
    c["omr"] = 1.0 - c["rho"]
    return _adadelta(_d(p), _d(g), _d(sq), _d(acc), c)


# ---- the fp32 models: the same formulas on fp32 tensors with fp32 scalars ---
def _f32(x):
    return float(torch.tensor(x, dtype=torch.float64).float())


def _f32_scalars(c):
    return {k: (_f32(x) if isinstance(x, float) else x) for k, x in c.items()}


def _complement(x, how):
    """1 - x as an fp32 number: rounded once from double, or (``how`` =
    "fp32", the parent commit's expression) formed in fp32 from float(x)."""
    if how == "fp32":
        return float(torch.tensor(1.0, dtype=F32) - torch.tensor(x, dtype=F32))
    return _f32(1.0 - x)


def model_sgd_step(p, g, buf=None, complement="rounded", **kw):
    c = {**SGD_DEFAULT, **kw}
    omd = _complement(c["dampening"], complement)
    c = _f32_scalars(c)
    c["omd"] = omd
    return _sgd(_f(p), _f(g), _f(buf), c)


def model_adam_step(p, g, m, v, vmax=None, *, step, device_step=False, complement="rounded", **kw):
    c = {**ADAM_DEFAULT, **kw}
    omb1, omb2 = _complement(c["beta1"], complement), _complement(c["beta2"], complement)
    if device_step:  # as the capturable kernel: powf on the fp32 beta and step
        b1, b2, st = (torch.tensor(x, dtype=F32) for x in (c["beta1"], c["beta2"], float(step)))
        bc1 = float(1.0 - torch.pow(b1, st))
        bc2_sqrt = float((1.0 - torch.pow(b2, st)).sqrt())
    else:
        bc1 = _f32(1.0 - c["beta1"] ** step)
        bc2_sqrt = _f32(math.sqrt(1.0 - c["beta2"] ** step))
    c = _f32_scalars(c)
    c["omb1"], c["omb2"] = omb1, omb2
    return _adam(_f(p), _f(g), _f(m), _f(v), _f(vmax), c, bc1, bc2_sqrt)


def model_adadelta_step(p, g, sq, acc, complement="rounded", **kw):
    c = {**ADADELTA_DEFAULT, **kw}
    omr = _complement(c["rho"], complement)
    c = _f32_scalars(c)
    c["omr"] = omr
    return _adadelta(_f(p), _f(g), _f(sq), _f(acc), c)


def model_sumsq(tensors):
    """Σx² in fp32 in the kernel's shape: per 8192-element chunk each of 256
    threads runs an fmaf chain over its <= 32 elements (vector layout: 8
    vectors of 4), a 64-lane butterfly, the 4 waves in order, then the chunks
    in list order (the kernel's atomics add them in any order)."""
    total = torch.zeros((), dtype=F32)
    for t in tensors:
        x = t.detach().flatten().cpu().double()
        for c0 in range(0, x.numel(), CHUNK):
            c = torch.zeros(CHUNK, dtype=torch.float64)
            n = min(CHUNK, x.numel() - c0)
            c[:n] = x[c0:c0 + n]
            c = c.view(8, 256, 4)
            acc = torch.zeros(256, dtype=F32)
            for w in range(8):
                for k in range(4):  # fmaf: exact product, one rounding
                    acc = (acc.double() + c[w, :, k] * c[w, :, k]).float()
            wv = acc.view(4, 64)
            off = 32
            while off:
                wv = wv[:, :off] + wv[:, off:2 * off]
                off >>= 1
            s = torch.zeros((), dtype=F32)
            for k in range(4):
                s = s + wv[k, 0]
            total = total + s
    return total


# ------------------------------------------------------------ tensor lists ---
PAD = 16
# (kind, size, element offset of the view behind its front padding)
LAYOUT = [("plain", 1, None), ("plain", 2, None), ("plain", 3, None), ("plain", 4, None), ("plain", 5, None),
          ("plain", 7, None), ("plain", CHUNK - 1, None), ("empty", 0, None), ("plain", CHUNK, None),
          ("view", 4099, 1), ("plain", CHUNK + 1, None), ("cl", (2, 8, 3, 3), None), ("view", 1027, 2),
          ("plain", 2 * CHUNK + 2, None), ("view", CHUNK + 3, 3), ("plain", 3 * CHUNK + 1, None)]
EMPTY = 7
SMALL_LAYOUT = [("plain", 5, None), ("plain", CHUNK + 9, None), ("plain", 1030, None)]
_SIGN_SEED = 12345


def _numel(size):
    return size if isinstance(size, int) else math.prod(size)


def _padded_view(vals, off, dev, dtype):
    n = vals.numel()
    buf = torch.empty(PAD + off + n + PAD, device=dev, dtype=dtype)
    bits(buf).fill_(SENTINEL[dtype])
    t = buf[PAD + off:PAD + off + n]
    t.copy_(vals)
    assert t.storage_offset() == PAD + off and t.data_ptr() % 16 == (off * t.element_size()) % 16
    return t


def ragged(dev, dtype, seed, lo=0.5, hi=2.0, signed=True, negate=False, offset=None, layout=LAYOUT):
    """The tensor list: numels 1, 2, 3, 4, 5, 7, 8191, 8192, 8193, 2·8192+2 and
    3·8192+1 (vector body, scalar tail, an exact chunk, a chunk boundary ±1,
    several chunks with a tail), an empty tensor in the middle, one
    channels_last 4-D tensor and three views at element offsets 1, 2 and 3
    behind 16 sentinel-filled elements of padding (16 more behind the view).
    Values: s_i · U(lo, hi) rounded to ``dtype``; the signs s_i depend on the
    position only, not on ``seed`` (``signed=False``: all positive;
    ``negate``: all flipped). ``offset`` = k makes every 1-D tensor a padded
    view at element offset k instead (k = 0: aligned, but with sentinels)."""
    gv = torch.Generator().manual_seed(seed)
    gs = torch.Generator().manual_seed(_SIGN_SEED)
    out = []
    for kind, size, off in layout:
        n = _numel(size)
        vals = lo + (hi - lo) * torch.rand(n, generator=gv)
        sign = torch.randint(0, 2, (n,), generator=gs).float() * 2 - 1
        if signed:
            vals = vals * sign
        if negate:
            vals = -vals
        if kind == "cl":
            t = vals.view(size).to(dev, dtype).contiguous(memory_format=torch.channels_last)
        elif kind == "empty":
            t = torch.empty(0, device=dev, dtype=dtype)
        elif offset is not None or kind == "view":
            t = _padded_view(vals, off if offset is None else offset, dev, dtype)
        else:
            t = vals.to(dev, dtype)
        out.append(t)
    return out


def paddings(tensors):
    """Bit patterns of the padding around every padded view in the list."""
    out = []
    for t in tensors:
        base = t._base
        if base is not None and t.numel() and base.dim() == 1 and base.numel() > t.numel():
            o = t.storage_offset()
            out.append(torch.cat([bits(base)[:o], bits(base)[o + t.numel():]]).clone())
    return out


def assert_paddings_intact(tensors, before, what=""):
    after = paddings(tensors)
    assert len(after) == len(before)
    for k, (a, b) in enumerate(zip(after, before)):
        assert torch.equal(a, b), f"{what}: padding of view {k} was overwritten"


# ------------------------------------------------------------------ cases ---
SGD_CASES = {
    "plain": dict(momentum=0.0),
    "momentum_first_step": dict(momentum=0.9, first=True),  # first_step True, then False
    "nesterov_wd": dict(momentum=0.9, nesterov=True, weight_decay=0.05),
    "dampening_maximize_scaled": dict(momentum=0.9, dampening=0.3, maximize=True, grad_scale=0.25),
}
ADAM_CASES = {
    "default": {},
    "coupled_wd": dict(weight_decay=0.1),
    "decoupled_wd": dict(weight_decay=0.1, decoupled=True),
    "amsgrad_decoupled_wd": dict(amsgrad=True, weight_decay=0.1, decoupled=True),
    "maximize_scaled_betas": dict(maximize=True, grad_scale=0.25, beta1=0.8, beta2=0.95),
    "eps_1e-3": dict(eps=1e-3),
    # zero moments, as at the start of training: exp_avg_sq is (1 - beta2)·g²
    # alone, so an error in the constant 1 - beta2 is not diluted by beta2·v
    "fresh_state": dict(fresh=True),
}
ADADELTA_CASES = {
    "default": {},
    "wd_maximize_scaled_rho": dict(weight_decay=0.1, maximize=True, grad_scale=0.5, rho=0.95),
}
CASES = {"sgd": SGD_CASES, "adam": ADAM_CASES, "adadelta": ADADELTA_CASES}
STEPS = 3
STEP_VALUES = [1, 2, 3, 10, 100, 1000, 100000]


def make_lists(kind, cfg, dev, dtype, offsets=None, layout=LAYOUT):
    """Parameters and state of ``kind`` ({name: list}); ``offsets`` maps a list
    name to the element offset at which all its tensors are carved."""
    offsets = offsets or {}
    mk = lambda name, seed, **kw: ragged(dev, dtype, seed, offset=offsets.get(name), layout=layout, **kw)  # noqa: E731
    L = {"p": mk("p", 1)}
    if kind == "sgd":
        if cfg.get("momentum", 0.0) != 0:
            L["buf"] = mk("buf", 2, lo=0.0, hi=0.0) if cfg.get("first") else mk("buf", 2, lo=0.5, hi=1.5)
    elif kind == "adam":
        z = dict(lo=0.0, hi=0.0) if cfg.get("fresh") else dict(lo=0.5, hi=1.5)
        L["m"] = mk("m", 2, **z)
        L["v"] = mk("v", 3, signed=False, **z)
        if cfg.get("amsgrad"):
            L["vmax"] = mk("vmax", 4, lo=0.5, hi=1.5, signed=False)
    else:
        L["sq"] = mk("sq", 2, lo=0.5, hi=1.5, signed=False)
        L["acc"] = mk("acc", 3, lo=0.01, hi=0.03, signed=False)
    return L


def make_grads(cfg, dev, dtype, it, offset=None, layout=LAYOUT):
    return ragged(dev, dtype, 100 + it, lo=0.05, hi=0.25, negate=bool(cfg.get("maximize")), offset=offset,
                  layout=layout)


def call_kernel(C, kind, cfg, L, g, it, steps=None, step=None):
    """One launch of _C.fused_sgd / fused_adam / fused_adadelta on the lists."""
    if kind == "sgd":
        c = {**SGD_DEFAULT, **{k: v for k, v in cfg.items() if k != "first"}}
        C.fused_sgd(L["p"], g, L.get("buf", []), c["lr"], c["momentum"], c["dampening"], c["weight_decay"],
                    c["nesterov"], c["maximize"], bool(cfg.get("first")) and it == 0, c["grad_scale"])
    elif kind == "adam":
        c = {**ADAM_DEFAULT, **{k: v for k, v in cfg.items() if k != "fresh"}}
        C.fused_adam(L["p"], g, L["m"], L["v"], L.get("vmax", []), c["lr"], c["beta1"], c["beta2"], c["eps"],
                     c["weight_decay"], float(it + 1 if step is None else step), c["amsgrad"], c["decoupled"],
                     c["maximize"], c["grad_scale"], [], steps or [])
    else:
        c = {**ADADELTA_DEFAULT, **cfg}
        C.fused_adadelta(L["p"], g, L["sq"], L["acc"], c["lr"], c["rho"], c["eps"], c["weight_decay"],
                         c["maximize"], c["grad_scale"])


def one_step(fn_kind, kind, cfg, before, g, i, it, step=None, **extra):
    """Reference ("ref") or fp32 model ("model") of tensor i's step from the
    stored tensors in ``before``: {output name: tensor}."""
    if kind == "sgd":
        kw = {k: v for k, v in cfg.items() if k != "first"}
        kw["first_step"] = bool(cfg.get("first")) and it == 0
        fn = ref_sgd_step if fn_kind == "ref" else model_sgd_step
        p, b = fn(before["p"][i], g[i], before["buf"][i] if "buf" in before else None, **kw, **extra)
        return {"p": p, "buf": b} if b is not None else {"p": p}
    if kind == "adam":
        fn = ref_adam_step if fn_kind == "ref" else model_adam_step
        st = (it + 1) if step is None else step
        p, m, v, vm = fn(before["p"][i], g[i], before["m"][i], before["v"][i],
                         before["vmax"][i] if "vmax" in before else None, step=st,
                         **{k: v for k, v in cfg.items() if k != "fresh"}, **extra)
        out = {"p": p, "m": m, "v": v}
        if vm is not None and "vmax" in before:
            out["vmax"] = vm
        return out
    fn = ref_adadelta_step if fn_kind == "ref" else model_adadelta_step
    p, sq, acc = fn(before["p"][i], g[i], before["sq"][i], before["acc"][i], **cfg, **extra)
    return {"p": p, "sq": sq, "acc": acc}


def run_case(C, kind, case, dev, dtype, offsets=None, layout=LAYOUT, steps=STEPS):
    """STEPS synchronised steps of the op on the tensor list: before each
    launch the reference takes the op's own stored tensors, so every output
    list of every step is one step away from exact inputs. Checks every list
    with ulp_bound, the gradients and all paddings bit for bit. Returns the
    largest relative error beyond the storage rounding per output."""
    cfg = CASES[kind][case]
    offsets = offsets or {}
    L = make_lists(kind, cfg, dev, dtype, offsets, layout)
    worst = {k: 0.0 for k in L}
    for it in range(steps):
        g = make_grads(cfg, dev, dtype, it, offsets.get("g"), layout)
        pads = paddings([t for l in L.values() for t in l] + g)
        before = {k: [t.clone() for t in l] for k, l in L.items()}
        g0 = [t.clone() for t in g]
        call_kernel(C, kind, cfg, L, g, it)
        for i in range(len(g)):
            exact = one_step("ref", kind, cfg, before, g, i, it)
            assert set(exact) == set(L)
            for name, want in exact.items():
                dev_ = assert_within(L[name][i], want, SLACK[kind][name], f"{kind}/{case} step {it} {name}[{i}]")
                worst[name] = max(worst[name], dev_)
            assert torch.equal(bits(g[i]), bits(g0[i])), f"gradient {i} was modified"
        assert_paddings_intact([t for l in L.values() for t in l] + g, pads, f"{kind}/{case} step {it}")
    return worst


def one_tensor(dev, dtype, n, seed, **kw):
    return ragged(dev, dtype, seed, layout=[("plain", n, None)], **kw)[0]


RANGES = [(0, 8190), (1, 8193), (2, 8194), (4, 20000), (8193, None)]


def run_range(C, dev, lo, hi):
    """fused_adam on view(-1)[lo:hi] of every list of one fp32 parameter with
    a bf16 shadow (Adam._step_ranges): oracle and shadow == p.to(bf16) bit for
    bit inside the range, everything bit-identical outside."""
    n = 3 * CHUNK + 1
    hi = n if hi is None else hi
    cfg = dict(weight_decay=0.1, decoupled=True)
    T = {"p": one_tensor(dev, F32, n, 1), "m": one_tensor(dev, F32, n, 2, lo=0.5, hi=1.5),
         "v": one_tensor(dev, F32, n, 3, lo=0.5, hi=1.5, signed=False)}
    g = one_tensor(dev, F32, n, 100, lo=0.05, hi=0.25)
    sh = one_tensor(dev, BF16, n, 9)  # not p.to(bf16): a write outside the range must show
    before = {k: t.clone() for k, t in T.items()}
    sh0 = sh.clone()
    r = lambda t: t.view(-1)[lo:hi]  # noqa: E731
    c = {**ADAM_DEFAULT, **cfg}
    C.fused_adam([r(T["p"])], [r(g)], [r(T["m"])], [r(T["v"])], [], c["lr"], c["beta1"], c["beta2"], c["eps"],
                 c["weight_decay"], 2.0, False, True, False, 1.0, [r(sh)], [])
    exact = dict(zip("pmv", ref_adam_step(r(before["p"]), r(g), r(before["m"]), r(before["v"]), step=2, **cfg)))
    for k in "pmv":
        assert_within(r(T[k]), exact[k], SLACK["adam"][k], f"range [{lo}:{hi}] {k}")
        for a, b in ((T[k][:lo], before[k][:lo]), (T[k][hi:], before[k][hi:])):
            assert torch.equal(bits(a), bits(b)), f"range [{lo}:{hi}]: {k} changed outside the range"
    assert torch.equal(bits(r(sh)), bits(r(T["p"]).to(BF16))), "shadow != p.to(bfloat16) inside the range"
    assert torch.equal(bits(sh[:lo]), bits(sh0[:lo])) and torch.equal(bits(sh[hi:]), bits(sh0[hi:])), \
        "shadow changed outside the range"


def sumsq_flag_cases(dev):
    """(name, tensor list, expected out[1]) for _C.sumsq: the flag tests the
    elements, so it stays 0 on finite input even where the sum overflows."""
    BIG, TAIL, VIEW1, LAST = 15, 10, 9, len(LAYOUT) - 1
    assert LAYOUT[TAIL][1] == CHUNK + 1 and LAYOUT[VIEW1][2] == 1

    def poisoned(dtype, i, k, val):
        xs = ragged(dev, dtype, 7)
        xs[i].view(-1)[k] = val
        return xs

    inf, nan = float("inf"), float("nan")
    yield "finite", ragged(dev, F32, 7), 0.0
    yield "finite_mixed", ragged(dev, F32, 7) + ragged(dev, BF16, 8), 0.0
    yield "inf_in_vector_body", poisoned(F32, BIG, 100, inf), 1.0
    yield "nan_in_scalar_tail", poisoned(F32, TAIL, CHUNK, nan), 1.0
    yield "neg_inf_last_element", poisoned(F32, LAST, -1, -inf), 1.0
    yield "nan_in_bf16_half_of_mixed", ragged(dev, F32, 7) + poisoned(BF16, 8, 4000, nan), 1.0
    yield "nan_in_offset_1_view", poisoned(F32, VIEW1, 2000, nan), 1.0


def check_sumsq_flags(C, dev):
    for name, xs, want in sumsq_flag_cases(dev):
        out = C.sumsq(xs)
        assert float(out[1]) == want, name
        if want == 0.0:
            assert math.isfinite(float(out[0])), name
    out = C.sumsq([torch.tensor([1e30], device=dev)])
    assert math.isinf(float(out[0])) and float(out[1]) == 0.0, "1e30: the sum overflows, no element is non-finite"


# ------------------------------------------- the measurement behind SLACK ---
def _rel_dev(model, exact):
    if exact.numel() == 0:
        return 0.0
    return float(((model.double() - exact).abs() / exact.abs()).max())


def measure(complement="rounded"):
    """Largest relative deviation of the fp32 models from fp64 per (kind,
    output) over all cases, dtypes and steps, the state carried forward as the
    model's result rounded to the dtype."""
    cpu = torch.device("cpu")
    table = {}
    for kind in CASES:
        for case, cfg in CASES[kind].items():
            for dtype in DTYPES:
                L = make_lists(kind, cfg, cpu, dtype)
                for it in range(STEPS):
                    g = make_grads(cfg, cpu, dtype, it)
                    nxt = {k: [] for k in L}
                    for i in range(len(g)):
                        exact = one_step("ref", kind, cfg, L, g, i, it)
                        model = one_step("model", kind, cfg, L, g, i, it, complement=complement)
                        for name in exact:
                            key = (kind, name)
                            table[key] = max(table.get(key, 0.0), _rel_dev(model[name], exact[name]))
                            nxt[name].append(model[name].to(dtype))
                    L = nxt
    # device steps: one launch, a different step per tensor
    cfg = {}
    for dtype in DTYPES:
        L = make_lists("adam", cfg, cpu, dtype)
        g = make_grads(cfg, cpu, dtype, 0)
        for i in range(len(g)):
            st = STEP_VALUES[i % len(STEP_VALUES)]
            exact = one_step("ref", "adam", cfg, L, g, i, 0, step=st)
            for mode, flag in (("adam_device_step", True), ("adam_host_step", False)):
                model = one_step("model", "adam", cfg, L, g, i, 0, step=st, device_step=flag, complement=complement)
                for name in exact:
                    key = (mode, name)
                    table[key] = max(table.get(key, 0.0), _rel_dev(model[name], exact[name]))
    # sum of squares and the scaled copy
    for dtype in DTYPES:
        xs = [t for t in ragged(cpu, dtype, 7, lo=0.05, hi=2.0) if t.numel()]
        exact = sum(float(t.double().pow(2).sum()) for t in xs)
        table[("sumsq", "out")] = max(table.get(("sumsq", "out"), 0.0), abs(float(model_sumsq(xs)) - exact) / exact)
        for t in xs:
            exact = t.double() * _f32(0.37)
            table[("scale", "x")] = max(table.get(("scale", "x"), 0.0), _rel_dev(t.float() * 0.37, exact))
    return table


if __name__ == "__main__":
    for how in ("rounded", "fp32"):
        print(f"complements: {how}")
        for (kind, name), dev_ in sorted(measure(how).items()):
            print(f"  {kind:18s} {name:5s} max rel deviation of the fp32 model {dev_:.3e}   x4 = {4 * dev_:.3e}")
