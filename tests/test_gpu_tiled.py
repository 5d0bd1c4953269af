"""Tiled inference on the MI355X (csrc/tiled.hip, mgunet.tiled) against tests/tiled_oracle.py: the gathers bit for bit against
numpy's reflect padding and ImagePreprocessor, the merge bit for bit on exact data and within the fp32 budget on random logits,
its independence of the chunking, predict_tiled against one existing-path forward per tile, and the stages downstream."""
import ctypes as C

import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
import tiled_oracle as TO
import tta_oracle as VO
from mgunet import _lib
from mgunet.tiled import TilePlan

pytestmark = pytest.mark.gpu

CFG = (3, 2, 8, 2)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def unet(dev, dtype=torch.float32, cfg=CFG, seed=3):
    m = mgunet.UNet(*cfg, compute_dtype=dtype)
    m.load_state_dict(O.make_unet_params(*cfg, seed=seed))
    return m.to(dev).eval()


def images(shape, dev, seed=7):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def run_chunks(plan, tiles_nhwc, chunk, C_, dev, is_prob=False, fused=True):
    """accumulate (ntiles, Th, Tw, C) `tiles_nhwc` in chunks of `chunk` tiles onto a canvas that starts as NaN"""
    canvas = torch.full((plan.B, plan.H, plan.W, C_), float("nan"), device=dev)
    labels = torch.full((plan.B, plan.H, plan.W), -1, device=dev, dtype=torch.int64)
    conf = torch.full((plan.B, plan.H, plan.W), float("nan"), device=dev)
    for t0 in range(0, plan.ntiles, chunk):
        part = tiles_nhwc[t0:t0 + chunk].contiguous()
        plan.accumulate(part, t0, canvas, labels if fused else None, conf if fused else None, is_prob=is_prob)
    if not fused:
        plan.finish(canvas, labels, conf)
    return canvas, labels, conf


# ---- 1. gather ---------------------------------------------------------------------------------------------------------------------

GATHER_CASES = [
    # (B, C, H, W), tile, overlap, layout
    ((2, 3, 64, 80), (32, 32), 8, "contiguous"),        # aligned and unaligned tile origins on unit-stride rows
    ((2, 3, 50, 70), (32, 48), 8, "channels_last"),     # strided input, non-square tile, shifted last tiles
    ((2, 3, 50, 70), (32, 48), 8, "sliced"),            # a window of a larger batch
    ((1, 3, 20, 90), (32, 48), 4, "contiguous"),        # H smaller than the tile: reflect padding below
    ((1, 2, 3, 1), (16, 8), 0, "contiguous"),           # folded several times; W == 1 reads index 0
    ((1, 3, 37, 45), (30, 21), 5, "contiguous"),        # Tw not a multiple of 4: scalar stores
]


@pytest.mark.parametrize("shape,tile,overlap,layout", GATHER_CASES)
def test_gather_is_reflect_pad_and_slice(cuda, shape, tile, overlap, layout):
    B, Cc, H, W = shape
    if layout == "sliced":
        x = images((B, Cc, H + 9, W + 11), cuda)[:, :, 4:4 + H, 6:6 + W]
    else:
        x = images(shape, cuda)
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
    assert x.is_contiguous() == (layout == "contiguous")
    plan = TilePlan(B, H, W, tile, overlap, "ramp", cuda)
    ref = TO.gather(x.cpu().numpy(), plan.Th, plan.Tw, plan.origins_y, plan.origins_x)
    assert ref.shape[0] == plan.ntiles
    got = plan.gather(x, 0, plan.ntiles).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    if plan.ntiles > 2:                                  # a chunk from the middle
        got = plan.gather(x, 1, plan.ntiles - 2).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref[1:-1].view(np.uint32))


@pytest.mark.parametrize("B,H,W,tile,overlap", [(1, 50, 70, (32, 48), 8), (2, 64, 64, (32, 32), 16), (1, 20, 30, (32, 32), 0)])
@pytest.mark.parametrize("bgr", [True, False])
def test_gather_u8_is_the_preprocessor_crop(cuda, B, H, W, tile, overlap, bgr):
    """Reference: ImagePreprocessor(resize_dim=(H, W)).preprocess(img) at native size (its resize is skipped at identity, so its
    output is exactly ToTensor + Normalize of the bytes), reflect-padded by numpy and sliced.  The preprocessor reads arrays as BGR;
    the RGB case feeds it the channel-reversed image."""
    rng = np.random.default_rng(H * W + B)
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    pre = mgunet.ImagePreprocessor(resize_dim=(H, W), mean=MEAN, std=STD)
    full = torch.stack([pre.preprocess(np.ascontiguousarray(im if bgr else im[..., ::-1])) for im in img])
    plan = TilePlan(B, H, W, tile, overlap, "ramp", cuda)
    ref = TO.gather(full.cpu().numpy(), plan.Th, plan.Tw, plan.origins_y, plan.origins_x)
    got = plan.gather_u8(torch.from_numpy(img).to(cuda), bgr, MEAN, STD, 0, plan.ntiles).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---- 2. merge on exact data --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cls", [1, 2, 3, 4, 5, 8, 16])
def test_merge_exact_on_one_hot_tiles(cuda, Cls):
    """24 x 24 images, 16 x 16 tiles, overlap 8, flat window: coverage 1, 2 and 4, weights 1, 1/2 and 1/4.  Logits 0 / -200 make the
    fp32 softmax exactly one-hot (expf(-200) = 0), so every probability is a multiple of 1/4 and must come out bit for bit."""
    one_hot_tiles_exact(cuda, Cls, 24)


def test_merge_exact_on_one_hot_tiles_odd_width(cuda):
    """The same on 24 x 23 images (column origins [0, 7]): two classes at an odd width run tile_accumulate_kernel<2, 1>, the one
    instantiation the even width above leaves to the random logits."""
    one_hot_tiles_exact(cuda, 2, 23)


def one_hot_tiles_exact(cuda, Cls, W):
    B, H, T, o = 2, 24, 16, 8
    plan = TilePlan(B, H, W, T, o, "flat", cuda)
    assert (plan.origins_y, plan.origins_x) == ([0, 8], [0, W - T])
    cover = np.outer(TO.coverage(H, T, plan.origins_y), TO.coverage(W, T, plan.origins_x))
    assert sorted(set(cover.ravel())) == [1, 2, 4]
    rng = np.random.default_rng(Cls)
    cls = rng.integers(0, Cls, (plan.ntiles, T, T))
    onehot = np.eye(Cls)[cls]                                            # (ntiles, T, T, C) float64
    logits = torch.from_numpy(((onehot - 1.0) * 200.0).astype(np.float32)).to(cuda)
    ref = TO.merge(onehot, B, H, W, T, T, o, "flat")
    assert np.array_equal(ref * 4, np.round(ref * 4)) and np.all(ref.sum(-1) == 1.0)
    ref32 = torch.from_numpy(ref.astype(np.float32)).to(cuda)
    for chunk, fused in ((plan.ntiles, True), (3, True), (3, False)):
        canvas, labels, conf = run_chunks(plan, logits, chunk, Cls, cuda, fused=fused)
        assert torch.equal(bits(canvas), bits(ref32)), (chunk, fused)
        assert torch.equal(labels, ref32.argmax(-1)) and torch.equal(conf, ref32.amax(-1))
        assert set(np.unique(canvas.cpu().numpy())) <= {0.0, 0.25, 0.5, 0.75, 1.0}


# ---- 3. merge on random logits -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", ["ramp", "flat"])
@pytest.mark.parametrize("Cls,W", [(2, 76), (2, 75), (3, 75), (4, 75), (7, 76), (1, 75), (8, 76), (16, 75)])
def test_merge_random_logits_against_float64(cuda, window, Cls, W):
    """52 x W images, 32 x 48 tiles, overlap 10: origins [0, 20] and [0, W - 48], both last tiles shifted back, at most four tiles
    per pixel.  Bound 3e-6: the 2e-6 test_none_is_the_plain_softmax allows an fp32 softmax against float64, plus at most four
    weighted additions and two weight roundings at <= 2^-24 each on values <= 1.
    The same at 16 classes, counted as tests/tta_oracle.py's bound() counts: one tile's fp32 softmax is within (C + 3) 2^-24 of
    float64 (0.37 for the subtraction of the maximum, 2 ulp of expf, the (C - 1)-term sum, one division) = 19 * 2^-24 = 1.13e-6,
    and a weighted mean with weights summing to 1 keeps that; each of at most four tiles adds a product and a sum rounding on
    values <= 1 (8), and the weight is a rounded product of two rounded table entries (3): 30 * 2^-24 = 1.8e-6 <= 3e-6, so the
    bar stays."""
    B, H, Th, Tw, o = 2, 52, 32, 48, 10
    plan = TilePlan(B, H, W, (Th, Tw), o, window, cuda)
    assert plan.origins_y == [0, 20] and plan.origins_x == [0, W - Tw] and 20 % (Th - o) and (W - Tw) % (Tw - o)
    logits = 3.0 * torch.randn((plan.ntiles, Th, Tw, Cls), generator=torch.Generator().manual_seed(Cls * W))
    ref = TO.merge(TO.softmax64(logits.numpy()), B, H, W, Th, Tw, o, window)
    assert np.abs(ref.sum(-1) - 1.0).max() <= 1e-6
    canvas, labels, conf = run_chunks(plan, logits.to(cuda), 3, Cls, cuda)
    d = float(np.abs(canvas.cpu().numpy().astype(np.float64) - ref).max())
    print(f"[tiled merge {window} C={Cls} W={W}] max|probs - oracle| = {d:.2e}")
    assert d <= 3e-6
    probs = canvas.permute(0, 3, 1, 2)
    assert torch.equal(labels, probs.argmax(1)) and torch.equal(conf, probs.amax(1))


@pytest.mark.parametrize("case", ["spread", "huge", "dead"])
@pytest.mark.parametrize("Cls", [2, 5])
def test_merge_extreme_logits_against_float64(cuda, case, Cls):
    """test_merge_random_logits_against_float64's geometry (W = 75) and bar on the logits that drive the shared pixel_softmax to
    expf underflow (spread), to magnitudes of 3e4 (huge) and to classes at -1e30 (dead: their canvas values are exactly 0)."""
    B, H, W, Th, Tw, o = 2, 52, 75, 32, 48, 10
    plan = TilePlan(B, H, W, (Th, Tw), o, "ramp", cuda)
    logits = VO.logits(case, [(plan.ntiles, Th, Tw)], Cls, seed=Cls + len(case))[0]
    ref = TO.merge(TO.softmax64(logits.numpy()), B, H, W, Th, Tw, o, "ramp")
    canvas, labels, conf = run_chunks(plan, logits.to(cuda), 3, Cls, cuda)
    assert not torch.isnan(canvas).any() and int(labels.min()) >= 0
    d = float(np.abs(canvas.cpu().numpy().astype(np.float64) - ref).max())
    print(f"[tiled merge {case} C={Cls}] max|probs - oracle| = {d:.2e}")
    assert d <= 3e-6
    if case == "dead":
        for c in VO.dead_classes(Cls):
            assert bool((canvas[..., c] == 0.0).all()), c
    probs = canvas.permute(0, 3, 1, 2)
    assert torch.equal(labels, probs.argmax(1)) and torch.equal(conf, probs.amax(1))


# ---- 4. chunk invariance -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Cls,W,is_prob", [(2, 100, False), (2, 99, False), (4, 99, False), (6, 100, False), (3, 99, True),
                                           (1, 99, False), (16, 100, False), (2, 100, True), (4, 99, True), (8, 100, True),
                                           (1, 99, True), (2, 99, True)])
def test_chunking_does_not_change_a_bit(cuda, Cls, W, is_prob):
    B, H, T, o = 2, 70, 32, 12
    plan = TilePlan(B, H, W, T, o, "ramp", cuda)
    t = torch.randn((plan.ntiles, T, T, Cls), generator=torch.Generator().manual_seed(W + Cls)).to(cuda)
    if is_prob:
        t = torch.softmax(t, -1)
    whole = run_chunks(plan, t, plan.ntiles, Cls, cuda, is_prob)
    assert not torch.isnan(whole[0]).any() and int(whole[1].min()) >= 0 and not torch.isnan(whole[2]).any()   # every pixel written
    for chunk in (1, 3, 7):
        part = run_chunks(plan, t, chunk, Cls, cuda, is_prob)
        assert all(torch.equal(bits(a), bits(b)) if a.is_floating_point() else torch.equal(a, b) for a, b in zip(whole, part)), chunk
    again = run_chunks(plan, t, 3, Cls, cuda, is_prob, fused=False)
    assert torch.equal(bits(whole[0]), bits(again[0])) and torch.equal(whole[1], again[1]) and torch.equal(bits(whole[2]), bits(again[2]))


# ---- 5. a single tile is the plain path --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (1, 3, 48, 80)])
def test_single_tile_is_predict_tta_none(cuda, shape):
    m = unet(cuda)
    x = images(shape, cuda)
    a = mgunet.predict_tiled(m, x, tile=shape[2:], overlap=8, transforms="none")
    b = mgunet.predict_tta(m, x, "none")
    for u, v in zip(a, b):
        assert u.shape == v.shape and u.dtype == v.dtype and u.stride() == v.stride()
        assert torch.equal(u, v)


@pytest.mark.parametrize("shape,tile", [((2, 3, 40, 52), 64), ((1, 3, 30, 80), (48, 96))])
def test_single_padded_tile_against_the_oracle(cuda, shape, tile):
    """An image smaller than the tile in both axes: one reflect-padded tile per image.  Reference: the existing-path forward of the
    numpy-padded image, softmax in float64, cropped back -- every weight is 1.  Bound 1e-5 as in the end-to-end test below (another
    batch composition per forward)."""
    m = unet(cuda)
    x = images(shape, cuda, seed=13)
    B, _, H, W = shape
    Th, Tw = (tile, tile) if isinstance(tile, int) else tile
    pad = torch.from_numpy(np.pad(x.cpu().numpy(), ((0, 0), (0, 0), (0, Th - H), (0, Tw - W)), mode="reflect")).to(cuda)
    with torch.no_grad():
        ref = torch.cat([torch.softmax(m(pad[b:b + 1])[0].double(), 1) for b in range(B)])[:, :, :H, :W]
    probs, labels, conf = mgunet.predict_tiled(m, x, tile=tile, overlap=8)
    check_outputs(probs, labels, conf, shape, CFG[1])
    d = float((probs.double() - ref).abs().max())
    print(f"[tiled padded single tile {shape} {tile}] max|probs - softmax64 of the padded forward| = {d:.2e}")
    assert d <= 1e-5


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------

E2E = dict(shape=(2, 3, 200, 264), tile=96, overlap=32)


def per_tile_reference(model, x, tile, overlap, window="ramp", hflip=False):
    """the oracle fed with one existing-path forward per tile (batch 1), softmax in float64"""
    B, _, H, W = x.shape
    oy, ox = TO.axis_origins(H, tile, overlap), TO.axis_origins(W, tile, overlap)
    out = []
    with torch.no_grad():
        for b in range(B):
            for y in oy:
                for x0 in ox:
                    crop = x[b:b + 1, :, y:y + tile, x0:x0 + tile].contiguous()
                    p = torch.softmax(model(crop)[0].double(), 1)
                    if hflip:
                        f = torch.softmax(model(torch.flip(crop, (3,)).contiguous())[0].double(), 1)
                        p = (p + torch.flip(f, (3,))) / 2
                    out.append(p[0].permute(1, 2, 0).cpu().numpy())
    return TO.merge(np.stack(out), B, H, W, tile, tile, overlap, window)


def check_outputs(probs, labels, conf, shape, Cls):
    B, _, H, W = shape
    assert probs.shape == (B, Cls, H, W) and probs.dtype == torch.float32
    assert probs.permute(0, 2, 3, 1).is_contiguous()
    assert labels.shape == (B, H, W) and labels.dtype == torch.int64
    assert conf.shape == (B, H, W) and conf.dtype == torch.float32
    assert torch.equal(labels, probs.argmax(1)) and torch.equal(conf, probs.amax(1))


@pytest.mark.parametrize("transforms", ["none", "hflip"])
def test_predict_tiled_against_separate_forwards(cuda, transforms):
    """1e-5: test_views_match_torch_composition's bar for the same model under another batch composition per forward."""
    m = unet(cuda)
    x = images(E2E["shape"], cuda, seed=21)
    ref = per_tile_reference(m, x, E2E["tile"], E2E["overlap"], hflip=transforms == "hflip")
    outs = []
    for per in (1, 5):
        probs, labels, conf = mgunet.predict_tiled(m, x, tile=E2E["tile"], overlap=E2E["overlap"], transforms=transforms, tiles_per_batch=per)
        check_outputs(probs, labels, conf, E2E["shape"], CFG[1])
        d = float(np.abs(probs.permute(0, 2, 3, 1).cpu().numpy().astype(np.float64) - ref).max())
        print(f"[tiled e2e {transforms} tiles_per_batch={per}] max|probs - per-tile oracle| = {d:.2e}")
        assert d <= 1e-5
        outs.append(probs)
    assert float((outs[0] - outs[1]).abs().max()) <= 2e-5


def test_predict_tiled_strided_and_u8_inputs(cuda):
    """A channels-last window of a larger batch gives what its contiguous copy gives; a uint8 image gives what the float batch
    ImagePreprocessor makes of it gives (the two gathers write the same tiles)."""
    m = unet(cuda)
    big = images((2, 3, 120, 150), cuda).contiguous(memory_format=torch.channels_last)
    x = big[:, :, 7:107, 9:139]
    a = mgunet.predict_tiled(m, x, tile=(64, 48), overlap=16, tiles_per_batch=4)
    b = mgunet.predict_tiled(m, x.contiguous(), tile=(64, 48), overlap=16, tiles_per_batch=4)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    img = np.random.default_rng(5).integers(0, 256, (100, 130, 3), dtype=np.uint8)
    full = mgunet.ImagePreprocessor(resize_dim=(100, 130)).preprocess(img).unsqueeze(0)
    a = mgunet.predict_tiled(m, img, tile=(64, 48), overlap=16, tiles_per_batch=4, bgr=True)
    b = mgunet.predict_tiled(m, full, tile=(64, 48), overlap=16, tiles_per_batch=4)
    c = mgunet.predict_tiled(m, torch.from_numpy(img).to(cuda)[None], tile=(64, 48), overlap=16, tiles_per_batch=3, bgr=True, mean=MEAN, std=STD)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert float((a[0] - c[0]).abs().max()) <= 2e-5
    small = mgunet.predict_tiled(m, img[:40, :30], tile=64, overlap=16, bgr=True)      # reflect-padded to one 64 x 64 tile
    check_outputs(*small, (1, 3, 40, 30), CFG[1])


def test_predict_tiled_bf16_model(cuda):
    """bf16 storage against the fp32 tiled run at test_bf16_model's bar in tests/test_gpu_tta.py: test_gpu_bf16's logit bounds
    (max 2.5e-2, mean 3e-3 of max|logit|) carried through the softmax (|d p| <= max_c |d logit_c| / 2; a weighted mean with weights
    summing to 1 keeps the bound), and >= 99 % label agreement."""
    x = images(E2E["shape"], cuda, seed=5)
    m32, m16 = unet(cuda), unet(cuda, torch.bfloat16)
    kw = dict(tile=E2E["tile"], overlap=E2E["overlap"], tiles_per_batch=5)
    p32, l32, _ = mgunet.predict_tiled(m32, x, **kw)
    p16, l16, c16 = mgunet.predict_tiled(m16, x, **kw)
    check_outputs(p16, l16, c16, E2E["shape"], CFG[1])
    with torch.no_grad():
        scale = float(m32(x)[0].abs().max())
    d = (p16 - p32).abs()
    agree = float((l16 == l32).double().mean())
    print(f"[tiled bf16] max {float(d.max()):.3e} mean {float(d.mean()):.3e} (max|logit| {scale:.2f}), labels agree {agree*100:.2f} %")
    assert float(d.max()) <= 0.5 * 2.5e-2 * scale and float(d.mean()) <= 3e-3 * scale
    assert agree >= 0.99


# ---- 7. downstream -----------------------------------------------------------------------------------------------------------------

def test_a_blob_across_a_seam_is_one_object(cuda):
    """Synthetic logits through the C-ABI path: a 40 x 56 scene with one rectangle lying across both seams of its 32 x 32 tiles
    (overlap 8: origins [0, 8] x [0, 24]) and a second one inside a single tile.  The tiles are the gathered crops of the scene's
    logits, so the merged labels are the scene and connected_components finds the two objects whole."""
    H, W, T, o = 40, 56, 32, 8
    scene = torch.zeros((1, H, W), dtype=torch.int64)
    scene[0, 4:36, 10:50] = 1
    scene[0, 0:3, 0:5] = 1
    lg = torch.stack([(scene == 0).float(), (scene == 1).float()], 1).to(cuda) * 10.0          # (1, 2, H, W)
    plan = TilePlan(1, H, W, T, o, "ramp", cuda)
    assert (plan.origins_y, plan.origins_x) == ([0, 8], [0, 24])
    tiles = plan.gather(lg, 0, plan.ntiles).permute(0, 2, 3, 1).contiguous()
    canvas, labels, conf = run_chunks(plan, tiles, 3, 2, cuda)
    assert torch.equal(labels.cpu(), scene)
    probs = canvas.permute(0, 3, 1, 2)
    for src in (labels, probs):
        table = mgunet.connected_components(src)
        assert table.counts.tolist() == [2]
        assert table.bbox.tolist() == [[0, 0, 5, 3], [10, 4, 50, 36]] and table.area.tolist() == [15, 32 * 40]
    scores = mgunet.object_scores(table, probs)
    p1 = float(torch.softmax(torch.tensor([0.0, 10.0]), 0)[1])
    assert scores.shape == (2,) and np.allclose(scores.cpu().numpy(), p1, atol=3e-6)
    shapes = mgunet.object_shapes(table)
    assert shapes.status.tolist() == [0, 0]


def test_downstream_stages_accept_a_tiled_run(cuda):
    m = unet(cuda)
    probs, labels, conf = mgunet.predict_tiled(m, images((2, 3, 150, 170), cuda, seed=3), tile=64, overlap=16)
    table = mgunet.connected_components(probs)
    assert torch.equal(table.labels != 0, labels != 0)
    N = table.class_id.numel()
    assert N > 1
    scores = mgunet.object_scores(table, probs)
    assert scores.shape == (N,) and float(scores.min()) >= 0.5 - 1e-6 and float(scores.max()) <= 1.0
    assert mgunet.object_shapes(table).status.numel() == N


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(cuda):
    m = unet(cuda)
    x = images((1, 3, 40, 40), cuda)
    with pytest.raises(TypeError, match="UNet"):
        mgunet.predict_tiled(torch.nn.Identity(), x, tile=32, overlap=8)
    with pytest.raises(RuntimeError, match="eval"):
        mgunet.predict_tiled(m.train(), x, tile=32, overlap=8)
    m.eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.predict_tiled(m, x.cpu(), tile=32, overlap=8)
    with pytest.raises(TypeError):
        mgunet.predict_tiled(m, x.double(), tile=32, overlap=8)
    with pytest.raises(TypeError):
        mgunet.predict_tiled(m, np.zeros((40, 40, 3), np.float32), tile=32, overlap=8)
    with pytest.raises(RuntimeError, match="channels"):
        mgunet.predict_tiled(m, x[:, :2], tile=32, overlap=8)
    with pytest.raises(ValueError, match="classes"):
        mgunet.predict_tiled(mgunet.UNet(3, 17, 8, 2).to(cuda).eval(), x, tile=32, overlap=8)
    with pytest.raises(ValueError, match="non-empty"):
        mgunet.predict_tiled(m, x[:0], tile=32, overlap=8)
    for bad in (32, 40, -1):
        with pytest.raises(ValueError, match="overlap"):
            mgunet.predict_tiled(m, x, tile=32, overlap=bad)
    with pytest.raises(ValueError, match="overlap"):
        mgunet.predict_tiled(m, x, tile=(32, 16), overlap=16)
    with pytest.raises(ValueError, match="window"):
        mgunet.predict_tiled(m, x, tile=32, overlap=8, window="hann")
    with pytest.raises(ValueError, match="transforms"):
        mgunet.predict_tiled(m, x, tile=32, overlap=8, transforms="rot90")
    with pytest.raises(ValueError, match="2\\*\\*depth"):
        mgunet.predict_tiled(m, x, tile=(32, 2), overlap=1)
    with pytest.raises(ValueError, match="uint8 images only"):
        mgunet.predict_tiled(m, x, tile=32, overlap=8, mean=MEAN, std=STD)
    a = mgunet.predict_tiled(m, x, tile=32, overlap=8)
    check_outputs(*a, (1, 3, 40, 40), CFG[1])


def test_c_abi_refusals_leave_the_context_usable(cuda):
    """Each bad call raises ValueError (MGU_ERR_INVALID) before anything is launched; the same context then runs a good call."""
    B, Cc, H, W, T, o = 1, 2, 40, 40, 32, 8
    plan = TilePlan(B, H, W, T, o, "ramp", cuda)
    x = images((B, Cc, H, W), cuda)
    buf = torch.empty((plan.ntiles, Cc, T, T), device=cuda)
    tiles = torch.zeros((plan.ntiles, T, T, Cc), device=cuda)
    canvas = torch.empty((B, H, W, Cc), device=cuda)
    labels = torch.empty((B, H, W), device=cuda, dtype=torch.int64)
    conf = torch.empty((B, H, W), device=cuda)
    st = (C.c_int64 * 4)(*x.stride())
    m3 = (C.c_float * 3)(*MEAN)
    u8 = torch.zeros((B, H, W, 3), device=cuda, dtype=torch.uint8)

    def gather(img=x, To=(T, T, o, o), strides=st, t0=0, n=plan.ntiles, out=buf):
        _lib.call("mgu_tile_gather", cuda, img, B, Cc, H, W, strides, *To, t0, n, out)

    def gather_u8(img=u8, To=(T, T, o, o), t0=0, n=plan.ntiles, out=None, mean=m3):
        out = torch.empty((plan.ntiles, 3, T, T), device=cuda) if out is None else out
        _lib.call("mgu_tile_gather_u8", cuda, img, B, H, W, 1, mean, m3, *To, t0, n, out)

    def accumulate(t=tiles, Cn=Cc, To=(T, T, o, o), wy=plan.wy, t0=0, n=plan.ntiles, acc=canvas, lab=labels, cf=conf):
        _lib.call("mgu_tile_accumulate", cuda, t, 0, B, Cn, H, W, *To, wy, plan.wx, t0, n, acc, lab, cf)

    bad = [
        lambda: gather(To=(T, T, T, o)), lambda: gather(To=(T, T, o, T + 3)), lambda: gather(To=(T, T, -1, o)),      # o >= T, o < 0
        lambda: gather(t0=1), lambda: gather(t0=-1, n=1), lambda: gather(n=0), lambda: gather(t0=plan.ntiles, n=1),  # range outside
        lambda: gather(img=None), lambda: gather(out=None), lambda: gather(strides=None),                                  # NULL buffers
        lambda: gather_u8(To=(T, T, T, o)), lambda: gather_u8(t0=2, n=plan.ntiles - 1), lambda: gather_u8(img=None), lambda: gather_u8(mean=None),
        lambda: accumulate(To=(T, T, o, T)), lambda: accumulate(Cn=17), lambda: accumulate(Cn=0), lambda: accumulate(t0=3, n=2),
        lambda: accumulate(t=None), lambda: accumulate(wy=None), lambda: accumulate(acc=None), lambda: accumulate(lab=None),
        lambda: _lib.call("mgu_tile_finish", cuda, canvas, B, 17, H, W, labels, conf),
        lambda: _lib.call("mgu_tile_finish", cuda, None, B, Cc, H, W, labels, conf),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert _lib.lib().mgu_last_error(_lib.context(cuda).handle), i
    gather()
    gather_u8()
    accumulate()
    _lib.call("mgu_tile_finish", cuda, canvas, B, Cc, H, W, labels, conf)
    torch.cuda.synchronize()
    assert torch.equal(buf, plan.gather(x, 0, plan.ntiles))
    assert float((canvas - 0.5).abs().max()) <= 1e-6 and int(labels.max()) == 0   # all-zero logits: both classes at 1/2, the first wins
