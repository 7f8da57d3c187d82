"""crop_resize_norm_kernel (csrc/kernels/augment.hip) against the fp64 oracle
of tests/augment_ref.py, and AugmentedBatches on the GPU.

Shapes are the smallest at which the kernel can go wrong: sources 1x1, 5x7,
17x33, 64x48 with M in {1, 4} (permuted and repeated index); S = 1, 2 (a row
shorter than one 8-element run), 7 (3S = 21: two full runs and a tail of 5,
rows and images off the 16-B boundary), 8 (all vector stores), 224 with two
samples (84 runs per row, three rows per workgroup pass, ten row tiles).
Every launch mixes flips and box kinds (augment_ref.boxes_for). All launches
and oracles are computed once and shared by the tests.
"""
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16


def _op(store, index, box, flip, S, dtype):
    from distributed_compute_pytorch_amd.ops import crop_resize_normalize

    return crop_resize_normalize(store, index, box, flip, S, R.MEAN, R.STD, dtype=dtype)


@pytest.fixture(scope="module")
def results(cuda):
    """{key: (case on the CPU, store on the GPU, fp32 output, bf16 output, oracle)}"""
    out = {}
    for key, case in R.all_cases().items():
        store, index, box, flip = case
        S = key[3]
        dstore = store.to(cuda)
        y32 = _op(dstore, index, box, flip, S, F32)
        y16 = _op(dstore, index, box, flip, S, BF16)
        out[key] = (case, dstore, y32, y16, R.oracle(store, index, box, flip, S))
    torch.cuda.synchronize()
    return out


def test_fp32_within_bound_of_oracle_every_element(results):
    bound = R.bound().view(1, 3, 1, 1)
    worst = 0.0
    for key, (case, _, y32, _, exact) in results.items():
        N, S = len(case[1]), key[3]
        assert y32.shape == (N, 3, S, S) and y32.dtype == F32
        err = (y32.double().cpu() - exact).abs()
        ratio = float((err / bound).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), f"{key}: {int((err > bound).sum())} of {err.numel()} elements outside " \
                                           f"the bound, worst {ratio:.2f} x bound"
    print(f"largest |err| / bound over all cases: {worst:.3f} (K = {R.K_ROUNDINGS})")


def test_identity_boxes_bit_equal_to_affine(results):
    """h == w == S: every weight is 0 and the sample passes through, so the
    output is fl(fl(v·a) + b) of the source pixel (no fma), mirrored when
    flipped."""
    a, b = (t.float().view(1, 1, 3) for t in R.affine64())
    checked = 0
    for key, (case, _, y32, _, _) in results.items():
        store, index, box, flip = case
        S = key[3]
        got = y32.cpu()
        for i in range(len(index)):
            y0, x0, h, w = box[i].tolist()
            if h != S or w != S:
                continue
            v = store[index[i], y0:y0 + S, x0:x0 + S].float()  # [S, S, 3]
            want = (v * a + b).permute(2, 0, 1)
            if flip[i]:
                want = want.flip(-1)
            assert torch.equal(got[i].view(torch.int32), want.contiguous().view(torch.int32)), (key, i)
            checked += 1
    assert checked >= 20  # S in {1, 2, 7, 8} on the sources with room, both flips


def test_bf16_is_the_fp32_output_rounded_once(results):
    for key, (_, _, y32, y16, _) in results.items():
        assert y16.dtype == BF16 and y16.shape == y32.shape
        assert torch.equal(y16.view(torch.int16), y32.to(BF16).view(torch.int16)), key


def test_layout_is_channels_last(results):
    for key, (_, _, y32, y16, _) in results.items():
        for y in (y32, y16):
            assert y.is_contiguous(memory_format=torch.channels_last), key
            assert y.permute(0, 2, 3, 1).is_contiguous(), key


def test_two_calls_bit_identical(results):
    for key in [(4, 17, 33, 7), (4, 64, 48, 8), (4, 64, 48, 224)]:
        (store, index, box, flip), dstore, y32, y16, _ = results[key]
        assert torch.equal(_op(dstore, index, box, flip, key[3], F32).view(torch.int32), y32.view(torch.int32))
        assert torch.equal(_op(dstore, index, box, flip, key[3], BF16).view(torch.int16), y16.view(torch.int16))


@pytest.mark.parametrize("S", [7, 8])
def test_out_of_range_box_and_index_equal_their_clamped_values(cuda, S):
    M, H, W = 4, 17, 33
    big = 2 ** 31 - 1
    store = R.make_store(M, H, W).to(cuda)
    box = torch.tensor([[-3, -2, H + 10, W + 10], [H + 5, W + 5, 0, -1], [5, 30, 3, 100], [-big, 4, big, 6],
                        [big, big, big, big], [2, -big - 1, -big - 1, big]], dtype=torch.int32)
    index = torch.tensor([-1, M + 5, 2, 2 ** 62, -2 ** 62, 1], dtype=torch.int64)
    flip = torch.tensor([0, 1, 1, 0, 1, 255], dtype=torch.uint8)
    cbox = torch.tensor([R.clamp_box(b, H, W) for b in box.tolist()], dtype=torch.int32)
    cindex = index.clamp(0, M - 1)
    assert cbox.tolist()[:3] == [[0, 0, H, W], [H - 1, W - 1, 1, 1], [5, 30, 3, 3]]
    for dtype, bits in ((F32, torch.int32), (BF16, torch.int16)):
        got = _op(store, index, box, flip, S, dtype)
        want = _op(store, cindex, cbox, flip.clamp(max=1), S, dtype)
        assert torch.equal(got.view(bits), want.view(bits))
    err = (_op(store, index, box, flip, S, F32).double().cpu() - R.oracle(store.cpu(), index, box, flip, S)).abs()
    assert bool((err <= R.bound().view(1, 3, 1, 1)).all())


def test_wrapper_rejects_bad_arguments(cuda):
    from distributed_compute_pytorch_amd._ext import C

    store = R.make_store(2, 5, 7).to(cuda)
    idx, box, flip = torch.zeros(2, dtype=torch.int64, device=cuda), torch.ones((2, 4), dtype=torch.int32,
                                                                                device=cuda), \
        torch.zeros(2, dtype=torch.uint8, device=cuda)
    ok = (store, idx, box, flip, 4, list(R.MEAN), list(R.STD), BF16)
    assert C.crop_resize_norm(*ok).shape == (2, 3, 4, 4)
    for k, bad in [(0, store.float()), (0, store[..., :2]), (0, store.permute(0, 2, 1, 3)), (1, idx.int()),
                   (1, idx.cpu()), (2, box[:1]), (2, box.long()), (3, flip[:1]), (4, 0), (4, 4097),
                   (5, [0.5, 0.5]), (6, [1.0, 0.0, 1.0]), (7, torch.float16)]:
        args = list(ok)
        args[k] = bad
        with pytest.raises(RuntimeError):
            C.crop_resize_norm(*args)


def test_fused_stem_accepts_the_output(cuda):
    """The kernel's bf16 tensor goes through the fused ResNet stem like the
    torch-made tensor with the same bits (the fp32 output rounded by torch, as
    the bf16 check establishes)."""
    from torch import nn

    from distributed_compute_pytorch_amd.ops.stem import fused_stem

    S = 32
    store, index, box, flip = R.make_case(4, 64, 48, S)
    dstore = store.to(cuda)
    xk = _op(dstore, index, box, flip, S, BF16)
    xt = _op(dstore, index, box, flip, S, F32).to(BF16).contiguous(memory_format=torch.channels_last)
    assert xk.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(xk.view(torch.int16), xt.view(torch.int16))
    # and it is the operation the reference path defines (bf16 rounding of a value within 2e-5)
    ref = _op(store, index, box, flip, S, BF16).to(cuda)
    torch.testing.assert_close(xk.float(), ref.float(), rtol=2 ** -7, atol=1e-4)
    outs = []
    for x in (xk, xt):
        torch.manual_seed(0)
        conv = nn.Conv2d(3, 64, 7, 2, 3, bias=False).to(cuda)
        bn = nn.BatchNorm2d(64).to(cuda)
        with torch.autocast("cuda", dtype=BF16):
            outs.append(fused_stem(x, conv, bn))
    assert outs[0].shape == (len(index), 64, S // 4, S // 4)
    # bit-equal inputs; the stem's BN sums are fp32 atomics, so not bit-equal outputs
    torch.testing.assert_close(outs[0].float(), outs[1].float(), rtol=2e-2, atol=2e-2)


# --------------------------------------------------------------- batches ---
def _batches(store_images, labels, device_store, cuda, seed, **kw):
    import distributed_compute_pytorch_amd as dcp
    from distributed_compute_pytorch_amd.utils import AugmentedBatches, ImageStore

    store = ImageStore(store_images, labels, device=cuda if device_store else None)
    sampler = dcp.DistributedSampler(store, num_replicas=1, rank=0, shuffle=True, seed=2)
    return AugmentedBatches(store, sampler, generator=torch.Generator().manual_seed(seed), device=cuda, **kw), sampler


def test_augmented_batches_host_and_device_store(cuda):
    from distributed_compute_pytorch_amd.ops import random_resized_crop_params

    M, H, W, B, S = 22, 20, 24, 4, 8
    images, labels = R.make_store(M, H, W, seed=5), torch.arange(M) * 3 % 10
    got = {}
    for device_store in (False, True):
        it, sampler = _batches(images, labels, device_store, cuda, seed=9, batch_size=B, size=S, drop_last=False)
        got[device_store] = list(it)
        assert len(got[device_store]) == len(it) == 6
        assert it.stats["batches"] == 6
        it.close()
    order = torch.tensor(list(sampler))
    g = torch.Generator().manual_seed(9)
    dimages = images.to(cuda)
    for k, ((xh, yh), (xd, yd)) in enumerate(zip(got[False], got[True])):
        idx = order[k * B:(k + 1) * B]
        assert xh.device == cuda and xh.dtype == BF16 and xh.shape == (len(idx), 3, S, S)
        assert xh.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(xh.view(torch.int16), xd.view(torch.int16)), k  # host store == device store
        assert torch.equal(yh.cpu(), labels[idx]) and torch.equal(yd.cpu(), labels[idx])
        box, flip = random_resized_crop_params(len(idx), H, W, generator=g)
        want = _op(dimages, idx, box, flip, S, BF16)  # the op called directly with the same parameters
        assert torch.equal(xh.view(torch.int16), want.view(torch.int16)), k


@pytest.mark.parametrize("device_store", [False, True])
def test_batch_stays_intact_while_later_ones_are_prepared(cuda, device_store):
    """Batch k is read only after batches k+1 and k+2 were requested (k+2
    reuses k's pinned slot): it still equals a run consumed in order."""
    M, H, W, B, S = 40, 20, 24, 8, 8
    images, labels = R.make_store(M, H, W, seed=6), torch.arange(M) % 10
    it, _ = _batches(images, labels, device_store, cuda, seed=4, batch_size=B, size=S)
    in_order = [(x.clone(), y.clone()) for x, y in it]
    it2, _ = _batches(images, labels, device_store, cuda, seed=4, batch_size=B, size=S)
    held = list(it2)  # all five requested before any is looked at
    torch.cuda.synchronize()
    assert len(held) == 5
    for (xa, ya), (xb, yb) in zip(in_order, held):
        assert torch.equal(xa.view(torch.int16), xb.view(torch.int16)) and torch.equal(ya, yb)
    assert len({x.data_ptr() for x, _ in held}) == 5 and len({y.data_ptr() for _, y in held}) == 5


def test_tiny_resnet_trains_from_augmented_batches(cuda):
    """Three graph-free steps of the tiny ResNet of the model tests
    (resnet18_like, fused kernels, bf16 autocast, fused SGD) on one batch of
    16 colour-coded images per epoch, freshly cropped and flipped each time.
    The step size is small enough for plain SGD to descend on every step (at
    lr = 0.05 the third step overshoots: 2.39, 1.48, 4.15)."""
    import torch.nn.functional as F

    import distributed_compute_pytorch_amd as dcp
    from distributed_compute_pytorch_amd.models import resnet18_like
    from distributed_compute_pytorch_amd.utils import AugmentedBatches, ImageStore

    torch.manual_seed(0)
    M, H, W = 16, 80, 72
    labels = torch.arange(M) % 4
    colour = torch.tensor([[230, 30, 30], [30, 230, 30], [30, 30, 230], [220, 220, 40]], dtype=torch.float32)
    images = (colour[labels].view(M, 1, 1, 3) + 12 * torch.randn(M, H, W, 3)).clamp(0, 255).to(torch.uint8)
    store = ImageStore(images, labels, device=cuda)
    it = AugmentedBatches(store, None, batch_size=M, size=64, generator=torch.Generator().manual_seed(1))
    model = resnet18_like(num_classes=10, fused_bn=True).to(cuda).to(memory_format=torch.channels_last)
    opt = dcp.optim.SGD(model.parameters(), lr=0.01)
    losses = []
    for epoch in range(3):
        it.set_epoch(epoch)
        for x, y in it:
            assert x.shape == (M, 3, 64, 64) and torch.equal(y.cpu(), labels)
            with torch.autocast("cuda", dtype=BF16):
                loss = F.cross_entropy(model(x), y)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    print("losses:", losses)
    assert len(losses) == 3 and all(torch.isfinite(torch.tensor(losses)))
    assert losses[0] > losses[1] > losses[2], losses
