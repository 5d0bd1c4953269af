"""GPU tier of the training augmentation (-m gpu): ImagePreprocessor(apply_augmentation=True).preprocess / preprocess_pair and
mgunet.RandomFlipRotate against PIL's own output (tests/golden/augment.npz, tools/make_augment_golden.py), bit for bit, and against
each other.  No PIL or torchvision at test time."""
import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalise(u8_hwc):
    """ToTensor + Normalize on the host, as torchvision does it"""
    t = torch.from_numpy(np.ascontiguousarray(u8_hwc)).permute(2, 0, 1).float().div(255)
    return (t - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)


def cases(golden):
    g = golden["augment"]
    for k in range(int(g["ncases"])):
        yield (g[f"{k}_src"], tuple(int(v) for v in g[f"{k}_dst"]), int(g[f"{k}_flip"]), float(g[f"{k}_angle"]), g[f"{k}_img"],
               g[f"{k}_msrc"], g[f"{k}_mask"], g[f"{k}_inb"])


def test_preprocess_augmented_equals_pil(cuda, golden):
    for src, dst, flip, angle, img, *_ in cases(golden):
        pre = mgunet.ImagePreprocessor(resize_dim=dst, apply_augmentation=True)
        ref = normalise(img)
        got = pre.preprocess(np.ascontiguousarray(src[:, :, ::-1]), augment=(flip, angle))     # arrays are BGR
        assert torch.equal(got.cpu(), ref), (dst, flip, angle)
        got = pre.preprocess(torch.from_numpy(np.ascontiguousarray(src[:, :, ::-1])).to(cuda), augment=(flip, angle))
        assert torch.equal(got.cpu(), ref)
        # straight into an image slot of an NHWC batch
        batch = torch.zeros((2,) + dst + (3,), device=cuda)
        pre.preprocess(np.ascontiguousarray(src[:, :, ::-1]), out=batch[1].permute(2, 0, 1), augment=(flip, angle))
        assert torch.equal(batch[1].permute(2, 0, 1).cpu(), ref) and float(batch[0].abs().max()) == 0.0


def test_preprocess_draws_like_the_reference(cuda, golden):
    src, dst = next(cases(golden))[:2]
    bgr = np.ascontiguousarray(src[:, :, ::-1])
    pre = mgunet.ImagePreprocessor(resize_dim=dst, apply_augmentation=True)
    for seed in (0, 3, 17):
        torch.manual_seed(seed)
        got = [pre.preprocess(bgr).cpu() for _ in range(4)]
        after = torch.rand(2)
        torch.manual_seed(seed)
        draws = [mgunet.draw_flip_rotate(0.5, 15) for _ in range(4)]
        assert torch.equal(torch.rand(2), after)
        for g_, d in zip(got, draws):
            assert torch.equal(g_, pre.preprocess(bgr, augment=d).cpu())
    # without augmentation nothing is drawn and the output is the plain path
    plain = mgunet.ImagePreprocessor(resize_dim=dst)
    torch.manual_seed(5)
    ref = plain.preprocess(bgr).cpu()
    nxt = torch.rand(2)
    torch.manual_seed(5)
    assert torch.equal(torch.rand(2), nxt)
    assert torch.equal(pre.preprocess(bgr, augment=(0, 0.0)).cpu(), ref)


@pytest.mark.parametrize("mask_fill", [0, -100])
def test_preprocess_pair_equals_pil(cuda, golden, mask_fill):
    nc = 4
    for src, dst, flip, angle, img, msrc, mask, inb in cases(golden):
        pre = mgunet.ImagePreprocessor(resize_dim=dst, apply_augmentation=True)
        gi, gm = pre.preprocess_pair(np.ascontiguousarray(src[:, :, ::-1]), msrc, nc, mask_fill=mask_fill, augment=(flip, angle))
        assert torch.equal(gi.cpu(), normalise(img))
        ref = np.where(inb == 255, np.clip(mask.astype(np.int64), 0, nc - 1), mask_fill)
        assert gm.dtype == torch.int64 and np.array_equal(gm.cpu().numpy(), ref), (dst, flip, angle)
    # the draw comes from `generator`
    src, dst, _, _, _, msrc = next(cases(golden))[:6]
    pre = mgunet.ImagePreprocessor(resize_dim=dst, apply_augmentation=True)
    a = pre.preprocess_pair(np.ascontiguousarray(src[:, :, ::-1]), msrc, nc, mask_fill, generator=torch.Generator().manual_seed(4))
    d = mgunet.draw_flip_rotate(0.5, 15, torch.Generator().manual_seed(4))
    b = pre.preprocess_pair(np.ascontiguousarray(src[:, :, ::-1]), msrc, nc, mask_fill, augment=d)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _batch(cuda, B, H, W, seed):
    """B preprocessed (not augmented) images and masks, with the sources they came from"""
    rng = np.random.default_rng(seed)
    srcs = [rng.integers(0, 256, (H + 7, W + 5, 3), dtype=np.uint8) for _ in range(B)]
    msrcs = [rng.integers(0, 5, (H + 3, W + 9), dtype=np.uint8) for _ in range(B)]
    pre = mgunet.ImagePreprocessor(resize_dim=(H, W))
    x = torch.stack([pre.preprocess(s) for s in srcs])
    y = torch.stack([pre.preprocess_mask(m, 3) for m in msrcs])
    return srcs, msrcs, x, y


def _per_image(srcs, msrcs, H, W, gen_seed, mask_fill, p=0.5, degrees=15):
    pre = mgunet.ImagePreprocessor(resize_dim=(H, W), apply_augmentation=True)
    g = torch.Generator().manual_seed(gen_seed)
    outs = []
    for s, m in zip(srcs, msrcs):
        outs.append(pre.preprocess_pair(s, m, 3, mask_fill=mask_fill, augment=mgunet.draw_flip_rotate(p, degrees, g)))
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


# every layout at the ragged / odd sizes; the flagship 8 x 512^2 batch in the layout the Trainer is given
@pytest.mark.parametrize("B,H,W,layout", [(B, H, W, lay) for B, H, W in [(3, 37, 53), (2, 45, 31), (4, 64, 64)]
                                          for lay in ("nchw", "channels_last", "nhwc_slot")] + [(8, 512, 512, "nchw")])
def test_batch_equals_preprocess_pair(cuda, B, H, W, layout):
    srcs, msrcs, x, y = _batch(cuda, B, H, W, seed=B * H + W)
    mask_fill = -100 if W % 2 else 0
    ref_x, ref_y = _per_image(srcs, msrcs, H, W, gen_seed=H, mask_fill=mask_fill)
    aug = mgunet.RandomFlipRotate(mask_fill=mask_fill)
    g = torch.Generator().manual_seed(H)
    if layout == "nchw":
        gx, gy = aug(x, y, generator=g)
        assert gx.is_contiguous()
    elif layout == "channels_last":
        xc = x.contiguous(memory_format=torch.channels_last)
        gx, gy = aug(xc, y, generator=g)
        assert gx.is_contiguous(memory_format=torch.channels_last)
    else:   # read from and write into (B, C, H, W) views of NHWC buffers with a spare image
        nin = torch.zeros((B + 1, H, W, 3), device=cuda)
        nin[1:] = x.permute(0, 2, 3, 1)
        nout = torch.full((B + 1, H, W, 3), 7.0, device=cuda)
        gx, gy = aug(nin[1:].permute(0, 3, 1, 2), y, generator=g, out=nout[1:].permute(0, 3, 1, 2))
        assert gx.data_ptr() == nout[1].data_ptr() and bool((nout[0] == 7.0).all())
    assert torch.equal(gx, ref_x) and torch.equal(gy, ref_y)
    # the images alone: same bits
    assert torch.equal(aug(x, generator=torch.Generator().manual_seed(H)), ref_x)


def test_batch_edge_cases(cuda):
    _, _, x, y = _batch(cuda, 4, 40, 36, seed=1)
    ident = mgunet.RandomFlipRotate(p=0.0, degrees=0)
    gx, gy = ident(x, y)
    assert torch.equal(gx, x) and torch.equal(gy, y)
    flip = mgunet.RandomFlipRotate(p=1.0, degrees=0)
    gx, gy = flip(x, y)
    assert torch.equal(gx, torch.flip(x, dims=[3])) and torch.equal(gy, torch.flip(y, dims=[2]))
    aug = mgunet.RandomFlipRotate(mask_fill=-100)
    a = aug(x, y, generator=torch.Generator().manual_seed(11))
    b = aug(x, y, generator=torch.Generator().manual_seed(11))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # rotated-in pixels: the normalised black pixel and the ignore label, together
    black = ((torch.zeros(3) / 255 - torch.tensor(MEAN)) / torch.tensor(STD)).to(cuda)
    big = mgunet.RandomFlipRotate(p=0.0, degrees=15, mask_fill=-100)
    g = torch.Generator().manual_seed(2)
    gx, gy = big(x, y, generator=g)
    filled = gy == -100
    assert bool(filled.any())
    for c in range(3):
        assert bool((gx[:, c][filled] == black[c]).all())
    assert bool((gy[~filled] >= 0).all())
    with pytest.raises(ValueError):
        aug(x[:, :2])
    with pytest.raises(ValueError):
        aug(x, y[:, :5])


def test_trainer_step_on_augmented_batch(cuda):
    cfg = (3, 2, 8, 2)
    B, H, W = 2, 32, 48
    srcs, msrcs, x, y = _batch(cuda, B, H, W, seed=3)
    y = y.clamp_max(1)

    def trainer():
        unet = mgunet.UNet(*cfg)
        unet.load_state_dict(O.make_unet_params(*cfg, seed=2))
        return mgunet.Trainer(unet.to(cuda), lr=1e-3)

    t = trainer()
    aug = mgunet.RandomFlipRotate(mask_fill=-100)
    loss = t.train_step(*aug(x, y, generator=torch.Generator().manual_seed(0)))
    t.check()
    assert bool(torch.isfinite(loss).all())
    # p=0, degrees=0: bitwise the un-augmented step
    t1, t2 = trainer(), trainer()
    l1 = t1.train_step(x, y)
    l2 = t2.train_step(*mgunet.RandomFlipRotate(p=0.0, degrees=0)(x, y))
    t1.check(), t2.check()
    assert torch.equal(l1, l2) and torch.equal(t1.flat, t2.flat)
