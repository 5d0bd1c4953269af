"""The scale / crop / colour augmentation kernels (csrc/augment_affine.hip) on the GPU against the numpy oracle
(tests/augment_affine_oracle.py) on the shared cases (tests/augment_affine_cases.py): images BITWISE (compared as int32 views), masks
exact.  Every shape with every transform alone and combined, B = 1 and 3 with other parameters per image, NCHW / NHWC-strided /
misaligned outputs, the luma sums at the edges of the luma kernel's tile, the launch counts, run-to-run equality, RandomAffineColor
under a seeded generator, and one Trainer.train_step on its output."""
import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
import augment_affine_cases as AC
import augment_affine_oracle as AO
from mgunet import _lib
from mgunet.preprocess import luma_sums

pytestmark = pytest.mark.gpu

T = 8192      # mgu_augment_luma_tile() of the library this suite was written against; test_tile_size holds the two together


def stage(c, out_hw):
    return mgunet.RandomAffineColor(out_hw, mean=AC.MEAN, std=AC.STD, fill=AC.FILL, mask_fill=AC.MASK_FILL, num_classes=c["num_classes"],
                                    bgr=c["bgr"])


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def make_out(cuda, layout, B, H, W):
    """-> (the (B, 3, H, W) view the stage writes, the tensor that owns its memory)"""
    if layout == "nchw":
        o = torch.full((B, 3, H, W), float("nan"), device=cuda)
        return o, o
    if layout == "nhwc":
        o = torch.full((B, H, W, 3), float("nan"), device=cuda)
        return o.permute(0, 3, 1, 2), o
    o = torch.full((B, 3, H, W + 5), 777.0, device=cuda)      # rows start 4 bytes off a 16-byte boundary, pitch W + 5
    return o[..., 1:W + 1], o


def run_case(cuda, tag, layout="nchw", with_masks=True):
    img, masks, table, c = AC.inputs(tag)
    out_hw = AC.SHAPES[c["shape"]][1]
    view, owner = make_out(cuda, layout, len(c["names"]), *out_hw)
    r = stage(c, out_hw)(torch.from_numpy(img).to(cuda), torch.from_numpy(masks).to(cuda) if with_masks else None, out=view,
                         params=torch.from_numpy(table).to(torch.int32))
    return (r if with_masks else (r, None)) + (owner,)


def test_tile_size(cuda):
    assert int(_lib.lib().mgu_augment_luma_tile()) == T


@pytest.mark.parametrize("tag", list(AC.CASES))
def test_images_bitwise_and_masks_exact(cuda, tag):
    want, _, _, wmask = AC.reference(tag)
    out, ms, _ = run_case(cuda, tag)
    assert out.dtype == torch.float32 and ms.dtype == torch.int64 and out.is_contiguous()
    assert np.array_equal(ms.cpu().numpy(), wmask), tag
    assert np.array_equal(bits(out), want.view(np.int32)), tag


@pytest.mark.parametrize("layout", ["nhwc", "misaligned"])
@pytest.mark.parametrize("tag", [f"{s}/{g}" for s in AC.SHAPES if s != "512" for g in ("one", "g8", "g1")] + ["512/three"])
def test_other_output_layouts_agree(cuda, tag, layout):
    want, _, _, wmask = AC.reference(tag)
    out, ms, owner = run_case(cuda, tag, layout)
    assert np.array_equal(bits(out), want.view(np.int32)) and np.array_equal(ms.cpu().numpy(), wmask), (tag, layout)
    if layout == "misaligned":                                  # nothing beside the view is written
        W = out.shape[3]
        assert bool((owner[..., 0] == 777.0).all()) and bool((owner[..., W + 1:] == 777.0).all())


@pytest.mark.parametrize("tag", ["64x64/one", "40x24/g8", "5x7/g2"])
def test_images_only(cuda, tag):
    out, ms, _ = run_case(cuda, tag, with_masks=False)
    assert ms is None and np.array_equal(bits(out), AC.reference(tag)[0].view(np.int32))


# ---- luma sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", AC.luma_shapes(T), ids=lambda hw: str(hw[0] * hw[1]))
def test_luma_sums_exact_at_the_tile_edges(cuda, hw, B):
    rng = np.random.default_rng(hw[0] * hw[1] + B)
    img = rng.integers(0, 256, (B,) + hw + (3,), dtype=np.uint8)
    img[-1] = 255                                                                  # the largest sum there is
    for bgr in (False, True):
        got = luma_sums(torch.from_numpy(img).to(cuda), bgr=bgr).cpu().tolist()
        assert got == [AO.luma_sum(img[b][..., ::-1] if bgr else img[b]) for b in range(B)], (hw, B, bgr)
    assert got[-1] == 256 * 255 * hw[0] * hw[1]
    # an image base that is not 16-byte aligned, and not 4-byte aligned either
    flat = torch.zeros(img.size + 16, dtype=torch.uint8, device=cuda)
    for off in (1, 6):
        v = flat[off:off + img.size].view(img.shape)
        v.copy_(torch.from_numpy(img))
        assert luma_sums(v).cpu().tolist() == [AO.luma_sum(img[b]) for b in range(B)], (hw, B, off)


@pytest.mark.parametrize("hw", AC.luma_shapes(T), ids=lambda hw: str(hw[0] * hw[1]))
def test_mean_luma_reaches_the_colour_step(cuda, hw):
    """contrast 0 turns every pixel into the image's mean luma: the main kernel reads the sums the luma kernel made"""
    rng = np.random.default_rng(hw[0] * hw[1])
    img = rng.integers(0, 256, (3,) + hw + (3,), dtype=np.uint8)
    img[1] = 255
    rows = [AC.IDENT_ROW[:6] + mgunet.color_matrix_q12(1.0, 0.0)[0] + (mgunet.color_matrix_q12(1.0, 0.0)[1],),
            AC.IDENT_ROW[:6] + mgunet.color_matrix_q12(1.0, 0.5)[0] + (mgunet.color_matrix_q12(1.0, 0.5)[1],), AC.row("limit_mix", hw, hw)]
    table = np.asarray(rows, np.int64)
    aug = mgunet.RandomAffineColor(hw, mean=AC.MEAN, std=AC.STD)
    out = aug(torch.from_numpy(img).to(cuda), params=torch.from_numpy(table).to(torch.int32))
    want = AO.augment(img, table, hw, AC.MEAN, AC.STD)[0]
    assert np.array_equal(bits(out), want.view(np.int32))


def count_launches(cuda, table, hw=(9, 11), B=2, masks=True):
    rng = np.random.default_rng(1)
    img = torch.from_numpy(rng.integers(0, 256, (B,) + hw + (3,), dtype=np.uint8)).to(cuda)
    m = torch.from_numpy(rng.integers(0, 3, (B,) + hw, dtype=np.uint8)).to(cuda) if masks else None
    aug = mgunet.RandomAffineColor((8, 12))
    ctx = _lib.context(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        aug(img, m, params=table)
        torch.cuda.synchronize()
        stats = _lib.read_kernel_stats(ctx)
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return {k["name"]: k["launches"] for k in stats}


def test_launch_counts(cuda):
    ident = torch.tensor([AC.IDENT_ROW] * 2, dtype=torch.int32)
    with_k = ident.clone()
    with_k[1, 15] = -300
    for masks in (True, False):
        assert count_launches(cuda, ident, masks=masks) == {"augment affine": 1}                       # need_mean = 0: no luma kernel
        assert count_launches(cuda, with_k, masks=masks) == {"augment luma": 1, "augment affine": 1}
    assert count_launches(cuda, ident.to(cuda)) == {"augment luma": 1, "augment affine": 1}            # a device table is not inspected


# ---- run to run, the generator, the trainer ---------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal(cuda):
    a, am, _ = run_case(cuda, "512/three")
    b, bm, _ = run_case(cuda, "512/three")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(am, bm)


def test_seeded_generator_equals_the_oracle_on_its_own_draw(cuda):
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (3, 45, 61, 3), dtype=np.uint8)
    masks = rng.integers(0, 4, (3, 45, 61), dtype=np.uint8)
    aug = mgunet.RandomAffineColor((40, 52), num_classes=3, fill=(10, 200, 30))
    table = aug.draw(3, (45, 61), generator=torch.Generator().manual_seed(21))
    assert len({tuple(r) for r in table.tolist()}) == 3 and bool((table[:, 15] != 0).any())
    out, ms = aug(torch.from_numpy(img).to(cuda), torch.from_numpy(masks).to(cuda), generator=torch.Generator().manual_seed(21))
    want, _, _, wm = AO.augment(img, table.numpy(), (40, 52), aug.mean, aug.std, masks=masks, fill=(10, 200, 30), mask_fill=-100, num_classes=3)
    assert np.array_equal(bits(out), want.view(np.int32)) and np.array_equal(ms.cpu().numpy(), wm)
    assert tuple(out.shape) == (3, 3, 40, 52) and tuple(ms.shape) == (3, 40, 52)


def test_bad_arguments_raise(cuda):
    aug = mgunet.RandomAffineColor((8, 8))
    img = torch.zeros(2, 9, 9, 3, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError, match="masks"):
        aug(img, torch.zeros(2, 9, 8, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError, match="out"):
        aug(img, out=torch.zeros(2, 3, 8, 9, device=cuda))
    with pytest.raises(ValueError, match="params"):
        aug(img, params=torch.zeros(3, 16, dtype=torch.int32))
    bad = torch.tensor([AC.IDENT_ROW] * 2, dtype=torch.int32)
    bad[0, 7] = (1 << 15) + 1
    with pytest.raises(ValueError, match="2\\^15"):
        aug(img, params=bad)


def test_trainer_step_on_augmented_batch(cuda):
    cfg = (3, 2, 8, 2)
    rng = np.random.default_rng(2)
    img = torch.from_numpy(rng.integers(0, 256, (2, 50, 70, 3), dtype=np.uint8)).to(cuda)
    masks = torch.from_numpy(rng.integers(0, 2, (2, 50, 70), dtype=np.uint8)).to(cuda)
    unet = mgunet.UNet(*cfg)
    unet.load_state_dict(O.make_unet_params(*cfg, seed=2))
    t = mgunet.Trainer(unet.to(cuda), lr=1e-3)
    aug = mgunet.RandomAffineColor((32, 48), scale=(0.5, 0.6), num_classes=2)          # zoomed out: fill, so ignore_index pixels
    x, y = aug(img, masks, generator=torch.Generator().manual_seed(0))
    assert bool((y == -100).any()) and bool((y >= 0).any()) and int(y.max()) <= 1
    loss = t.train_step(x, y)
    t.check()
    assert bool(torch.isfinite(loss).all())
