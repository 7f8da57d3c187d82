"""Shared by the image augmentation tests: an fp64 oracle of crop + bilinear
resize + flip + normalise written from the formula (not from F.interpolate),
the per-element bound the kernel's fp32 output is held to, a plain loop of
torchvision's RandomResizedCrop.get_params, and the GPU test cases. Nothing
here imports the package under test.

Oracle. Output column ox of a crop (y0, x0, h, w) resized to S x S samples
the source at x0 + n / 2S with n = (2·ox' + 1)·w − S, where ox' = S−1−ox for a
flipped sample (align_corners=False: (ox' + 1/2)·w/S − 1/2). q = floor(n / 2S)
and r = n − 2S·q are Python integers (// floors negative n too), the neighbour
pair is (q, q + 1) clamped into [0, w), the weight of the second is r / 2S.
Rows likewise. The four samples are blended in fp64:

    top = v00 + wx·(v01 − v00),  bot = v10 + wx·(v11 − v10)
    out = (top + wy·(bot − top))·a_c + b_c

with a_c = fp32(1 / (255·std_c)) and b_c = fp32(−mean_c / std_c), the values
the kernel receives. Boxes are first clamped into the image and indices into
[0, M), which is the operation's defined behaviour.

Bound. |kernel fp32 − oracle| <= K · 2⁻²⁴ · (255·|a_c| + |b_c|) on every
element. K = 8 is the number of fp32 roundings csrc/kernels/augment.hip
performs per element, counted from its code:

    1  wx = fp32(r_x / 2S)                    (division)
    2  wy = fp32(r_y / 2S)                    (division)
    3  top = fmaf(wx, v01 − v00, v00)         (the difference of two bytes is exact)
    4  bot = fmaf(wx, v11 − v10, v10)
    5  d   = bot − top
    6  val = fmaf(wy, d, top)
    7  t   = val · a_c
    8  out = t + b_c

Every intermediate of 1-6 is a weight in [0, 1) or a pixel-domain value of
magnitude <= 255, so a rounding there moves the pixel value by at most
2⁻²⁴·255 and the output by |a_c| times that (3 and 4 enter through the convex
combination of step 6, so together they count once: 8 is an upper bound, the
tight count is 7); rounding 7 is at most 2⁻²⁴·255·|a_c| and rounding 8 at most
2⁻²⁴·(255·|a_c| + |b_c|). Products of two rounding errors are of order 2⁻⁴⁸
and sit inside the slack between 7 and 8. The bf16 output is not bounded
separately: it is the same value rounded once more (tested bit for bit).
"""
import math

import torch

K_ROUNDINGS = 8
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def affine64(mean=MEAN, std=STD):
    """(a, b) as the kernel receives them (rounded to fp32 once), in fp64."""
    a = torch.tensor([1.0 / (255.0 * s) for s in std], dtype=torch.float64).float().double()
    b = torch.tensor([-m / s for m, s in zip(mean, std)], dtype=torch.float64).float().double()
    return a, b


def bound(mean=MEAN, std=STD):
    """Per-channel bound [3] on |fp32 output − oracle|."""
    a, b = affine64(mean, std)
    return K_ROUNDINGS * 2.0 ** -24 * (255.0 * a.abs() + b.abs())


def clamp_box(box, H, W):
    y0, x0, h, w = (int(v) for v in box)
    y0, x0 = min(max(y0, 0), H - 1), min(max(x0, 0), W - 1)
    return y0, x0, min(max(h, 1), H - y0), min(max(w, 1), W - x0)


def taps(S, length, flipped=False):
    """Per output index: (first neighbour, second neighbour, weight of the
    second as the exact pair (r, 2S)), in integers."""
    lo, hi, rem = [], [], []
    for o in range(S):
        o = S - 1 - o if flipped else o
        n = (2 * o + 1) * length - S
        q, r = n // (2 * S), n % (2 * S)  # Python: floor and a remainder in [0, 2S)
        assert n == q * 2 * S + r and 0 <= r < 2 * S
        lo.append(min(max(q, 0), length - 1))
        hi.append(min(max(q + 1, 0), length - 1))
        rem.append(r)
    return lo, hi, rem


def oracle(store, index, box, flip, S, mean=MEAN, std=STD):
    """fp64 [N, 3, S, S] of the operation on a CPU uint8 store [M, H, W, 3]."""
    M, H, W, _ = store.shape
    a, b = affine64(mean, std)
    out = torch.empty((len(index), 3, S, S), dtype=torch.float64)
    for i, (row, bx, fl) in enumerate(zip(index.tolist(), box.tolist(), flip.tolist())):
        y0, x0, h, w = clamp_box(bx, H, W)
        img = store[min(max(row, 0), M - 1)].double()
        ylo, yhi, ry = taps(S, h)
        xlo, xhi, rx = taps(S, w, flipped=bool(fl))
        ylo, yhi = torch.tensor(ylo) + y0, torch.tensor(yhi) + y0
        xlo, xhi = torch.tensor(xlo) + x0, torch.tensor(xhi) + x0
        wy = (torch.tensor(ry, dtype=torch.float64) / (2 * S)).view(S, 1, 1)
        wx = (torch.tensor(rx, dtype=torch.float64) / (2 * S)).view(1, S, 1)
        v00, v01 = img[ylo][:, xlo], img[ylo][:, xhi]  # [S, S, 3]
        v10, v11 = img[yhi][:, xlo], img[yhi][:, xhi]
        top = v00 + wx * (v01 - v00)
        bot = v10 + wx * (v11 - v10)
        out[i] = ((top + wy * (bot - top)) * a + b).permute(2, 0, 1)
    return out


# ------------------------------------------- torchvision's get_params loop ---
def rrc_loop(u, uf, H, W, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip=0.5):
    """RandomResizedCrop.get_params sample by sample, the random numbers taken
    from u [n, 10, 4] (area, log-ratio, top, left per attempt) and uf [n]."""
    boxes, flips = [], []
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for s in range(u.shape[0]):
        got = None
        for k in range(10):
            u0, u1, u2, u3 = (float(v) for v in u[s, k])
            area = float(H * W) * (scale[0] + (scale[1] - scale[0]) * u0)
            r = math.exp(lo + (hi - lo) * u1)
            w, h = int(round(math.sqrt(area * r))), int(round(math.sqrt(area / r)))
            if 0 < w <= W and 0 < h <= H:
                got = (min(int(math.floor(u2 * (H - h + 1))), H - h), min(int(math.floor(u3 * (W - w + 1))), W - w),
                       h, w)
                break
        if got is None:
            in_ratio = float(W) / float(H)
            if in_ratio < min(ratio):
                w, h = W, int(round(W / min(ratio)))
            elif in_ratio > max(ratio):
                h, w = H, int(round(H * max(ratio)))
            else:
                w, h = W, H
            got = ((H - h) // 2, (W - w) // 2, h, w)
        boxes.append(got)
        flips.append(1 if float(uf[s]) < p_flip else 0)
    return torch.tensor(boxes, dtype=torch.int32), torch.tensor(flips, dtype=torch.uint8)


# ------------------------------------------------------------------ cases ---
SOURCES = [(1, 1), (5, 7), (17, 33), (64, 48)]
SIZES = [1, 2, 7, 8]


def make_store(M, H, W, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + H * 37 + W)
    return torch.randint(0, 256, (M, H, W, 3), dtype=torch.uint8, generator=g)


def boxes_for(H, W, S):
    """The boxes of one launch: the whole image, a 1x1 box, one box touching
    each corner, a downscale (w > S), an upscale (w < S) and the identity
    (h == w == S) where the image has room for them; clamped duplicates drop
    nothing (a small image simply repeats boxes)."""
    hh, ww = max(1, (H + 1) // 2), max(1, (2 * W + 2) // 3)
    bx = [(0, 0, H, W), (H // 2, W // 3, 1, 1),
          (0, 0, hh, ww), (0, W - ww, hh, ww), (H - hh, 0, hh, ww), (H - hh, W - ww, hh, ww)]
    if W > S and H > S:
        bx.append((H - (S + 1), 0, S + 1, min(W, 2 * S + 1)))  # downscale, odd ratio
    if S > 1:
        bx.append((H // 3, W // 4, min(H - H // 3, S - 1), min(W - W // 4, max(1, S // 2))))  # upscale
    if S <= H and S <= W:
        bx += [((H - S) // 2, (W - S) // 2, S, S), (H - S, W - S, S, S)]  # identity
    return bx


def make_case(M, H, W, S, boxes=None):
    """(store, index, box, flip) on the CPU. The index is a permutation of the
    rows followed by repeats; flips alternate, starting with a flipped sample
    for odd H so that both parities of every box kind occur over the sources."""
    bx = boxes_for(H, W, S) if boxes is None else boxes
    n = len(bx)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(M + H + S)).tolist()
    index = torch.tensor([perm[i % M] if i < M else perm[(i * 3) % M] for i in range(n)], dtype=torch.int64)
    flip = torch.tensor([(i + H) % 2 for i in range(n)], dtype=torch.uint8)
    return make_store(M, H, W), index, torch.tensor(bx, dtype=torch.int32), flip


def all_cases():
    """{(M, H, W, S): case}: every source x M in {1, 4} x S in {1, 2, 7, 8},
    plus S = 224 with two samples (a whole image and a flipped crop)."""
    cases = {}
    for H, W in SOURCES:
        for M in (1, 4):
            for S in SIZES:
                cases[(M, H, W, S)] = make_case(M, H, W, S)
    cases[(4, 64, 48, 224)] = make_case(4, 64, 48, 224, boxes=[(0, 0, 64, 48), (5, 3, 40, 29)])
    return cases
