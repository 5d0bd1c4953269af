"""The image input / output kernels of csrc/imageops.hip on the device against the cases of tests/image_io_cases.py: PIL's resample and
the normalisation against PIL itself, the mask resize / Sobel / histogram equalisation / colour map against the oracle on inputs built
so that the arithmetic decides the result (tests/test_image_io_cases_host.py shows what each case has and which wrong kernel it
rejects), the patch means against exact integer sums, the gather against its definition, and the fp32 bilinear resize against the
float64 blend with a per-element bar computed by the reference.  Every byte and integer comparison is exact; the resize bar is the
only tolerance.  cv2 is not installed: the colour conversions and equalizeHist are held to the oracle's restatement, not the library."""
import ctypes as C

import numpy as np
import pytest
import torch

import image_io_cases as IC
import mgunet
import mgunet_oracle as O
from mgunet import _lib

pytestmark = pytest.mark.gpu


def _pre(dst):
    return mgunet.ImagePreprocessor(resize_dim=dst, mean=IC.MEAN, std=IC.STD)


# ---- 1. PIL resample + normalise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", IC.RESAMPLE_PAIRS)
def test_resample_and_normalise_equal_pil(cuda, src, dst):
    pre = _pre(dst)
    for content in IC.RESAMPLE_CONTENTS:
        for layout in IC.RESAMPLE_LAYOUTS:
            img = IC.resample_image(content, src, layout)
            ref = IC.resample_reference(img, dst, layout)
            if layout == "rgb":                       # arrays are BGR to the mirror (cv2.imread order): hand it the flipped image
                got = pre.preprocess(np.ascontiguousarray(img[:, :, ::-1]))
            else:
                got = pre.preprocess(img)
            assert tuple(got.shape) == (3,) + dst
            assert torch.equal(got.cpu(), ref), (content, layout, int((got.cpu() != ref).sum()))


def _call_preprocess(cuda, img, bgr, dst, out):
    """the C entry point itself: bgr = 0 reads the channels in place"""
    d = torch.from_numpy(np.ascontiguousarray(img if img.ndim == 3 else img[:, :, None])).to(cuda)
    mean, std = (C.c_float * 3)(*IC.MEAN), (C.c_float * 3)(*IC.STD)
    _lib.call("mgu_preprocess_image_u8", cuda, d, d.shape[0], d.shape[1], d.shape[2], bgr, dst[0], dst[1], mean, std, out, *out.stride())


@pytest.mark.parametrize("src,dst", [((97, 61), (33, 127)), ((1080, 3), (2, 2)), ((64, 64), (64, 64)), ((1, 1), (5, 7))])
def test_resample_rgb_order_and_a_strided_slot_between_nans(cuda, src, dst):
    img = IC.resample_image("noise", src, "rgb")
    ref = IC.resample_reference(img, dst, "rgb")
    batch = torch.full((3, dst[0], dst[1], 4), float("nan"), device=cuda)          # NHWC slots, one spare channel
    slot = batch[1, :, :, :3].permute(2, 0, 1)
    _call_preprocess(cuda, img, 0, dst, slot)
    assert torch.equal(slot.cpu(), ref)
    assert bool(torch.isnan(batch[0]).all()) and bool(torch.isnan(batch[2]).all()) and bool(torch.isnan(batch[1, :, :, 3]).all())
    plain = torch.full((3,) + dst, float("nan"), device=cuda)
    _call_preprocess(cuda, img, 0, dst, plain)
    assert torch.equal(plain.cpu(), ref)


def test_resample_workspace_reuse_large_then_small(cuda):
    big = IC.resample_image("noise", (600, 500), "bgr")
    pre_big = _pre((384, 320))
    assert torch.equal(pre_big.preprocess(big).cpu(), IC.resample_reference(big, (384, 320), "bgr"))
    for src, dst in (((7, 5), (1, 1)), ((2, 3), (64, 64)), ((1080, 3), (2, 2))):
        for content in ("full", "noise"):
            small = IC.resample_image(content, src, "bgr")
            ref = IC.resample_reference(small, dst, "bgr")
            assert torch.equal(_pre(dst).preprocess(small).cpu(), ref), (src, dst, content)
            pre_big.preprocess(big)                                                     # dirty the shared workspace again
            assert torch.equal(_pre(dst).preprocess(small).cpu(), ref), (src, dst, content)


# ---- 2. mask resize ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", IC.MASK_PAIRS)
def test_mask_resize_equals_the_double_index_rule(cuda, src, dst):
    m = IC.mask_image(src)
    pre = _pre(dst)
    for nc in IC.MASK_CLASSES:
        got = pre.preprocess_mask(m, nc)
        assert got.dtype == torch.int64 and tuple(got.shape) == dst
        ref = O.preprocess_mask(m, dst, nc)
        assert torch.equal(got.cpu(), ref), (nc, int((got.cpu() != ref).sum()))


# ---- 3. Sobel -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IC.sobel_cases()))
def test_sobel_bit_exact(cuda, name):
    img = IC.sobel_cases()[name]
    got = mgunet.EdgeDetector().sobel_edges(img)
    ref = O.sobel_edges(img)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    assert np.array_equal(got, ref), (name, int((got != ref).sum()))
    if name == "tie_dense":
        assert np.array_equal(got, IC.sobel_exact(img))
    dev = mgunet.EdgeDetector().sobel_edges(torch.from_numpy(img).to(cuda))        # a device tensor in, a device tensor out
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), ref)


# ---- 4. histogram equalisation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IC.histeq_cases()))
def test_equalize_hist_bit_exact(cuda, name):
    img = IC.histeq_cases()[name]
    got = mgunet.HistogramEqualizer().equalize_histogram_rgb(img)
    ref = O.equalize_histogram_rgb(img)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    assert np.array_equal(got, ref), (name, int((got != ref).sum()))


def test_sobel_and_equalize_hist_where_the_launches_stride(cuda):
    """2 097 152 pixels: the histogram launch (capped at 1024 blocks) strides 8 times, the others (capped at 2048) 4 times"""
    img = IC.histeq_big()
    assert img.shape[0] * img.shape[1] == 1024 * 256 * 8
    dev = torch.from_numpy(img).to(cuda)
    h = mgunet.HistogramEqualizer().equalize_histogram_rgb(dev).cpu().numpy()
    s = mgunet.EdgeDetector().sobel_edges(dev).cpu().numpy()
    assert np.array_equal(h, O.equalize_histogram_rgb(img))
    assert np.array_equal(s, O.sobel_edges(img))


# ---- 5. patch means, colour map, gather -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,Cc,patch", IC.PATCH_MEAN_CASES)
def test_patch_mean_is_the_exact_sum_rounded_once(cuda, H, W, Cc, patch):
    img = IC.patch_mean_image(H, W, Cc)
    for per_channel in (False, True):
        got = mgunet.patch_features_u8(img[:, :, 0] if Cc == 1 and per_channel else img, patch, per_channel)
        ref = IC.patch_mean_exact(img, patch, per_channel)
        assert got.shape == ref.shape and torch.equal(got.cpu(), ref), (per_channel, float((got.cpu() - ref).abs().max()))
    full = IC.patch_mean_image(H, W, Cc, full=True)
    assert torch.equal(mgunet.patch_features_u8(full, patch, True).cpu(), IC.patch_mean_exact(full, patch, True))


def test_patch_mean_sum_above_two_to_the_31(cuda):
    H, W, Cc, patch = IC.PATCH_MEAN_FULL
    full = IC.patch_mean_image(H, W, Cc, full=True)
    for per_channel in (False, True):
        got = mgunet.patch_features_u8(full, patch, per_channel)
        assert torch.equal(got.cpu(), IC.patch_mean_exact(full, patch, per_channel)), per_channel
    assert float(mgunet.patch_features_u8(full, patch, False)[0, 0]) > 0


def test_patch_mean_sum_above_two_to_the_32(cuda):
    """the largest patch the entry point takes, full of 255 over 3 channels: the sum 12 834 570 240 needs more than 32 bits, the mean is
    255 exactly.  (Only this size can show a 32-bit accumulator; the image is made on the device.)"""
    side, Cc = IC.PATCH_MEAN_WIDE
    full = torch.full((side, side, Cc), 255, dtype=torch.uint8, device=cuda)
    assert torch.equal(mgunet.patch_features_u8(full, side, False).cpu(), torch.tensor([[255.0]]))
    assert torch.equal(mgunet.patch_features_u8(full, side, True).cpu(), torch.full((1, Cc), 255.0))


@pytest.mark.parametrize("name,patch", [("tie_dense", 8), ("tie_dense", 16), ("cube", 16), ("cube", 32)])
def test_batched_patch_path_equals_the_per_image_composition(cuda, name, patch):
    """patch_inputs.hip shares imgmath.h: its byte columns on the adversarial images, against the single-image kernels tested above"""
    img = torch.from_numpy({"tie_dense": IC.tie_dense, "cube": IC.colour_cube}[name]()).to(cuda)
    batch = torch.stack([img, img.flip(1), img])                                    # three tables / maxima, the outer two equal
    for per_channel in (True, False):
        rows = []
        for one in batch:
            sob = mgunet.patch_features_u8(mgunet.EdgeDetector().sobel_edges(one), patch)
            eq = mgunet.patch_features_u8(mgunet.HistogramEqualizer().equalize_histogram_rgb(one), patch, per_channel)
            rows.append(torch.cat([sob, eq], 1))
        ref = torch.cat(rows, 0)
        got = mgunet.patch_node_features(batch, patch, per_channel=per_channel, pad_to=1)
        assert got.shape == ref.shape and torch.equal(got, ref), (per_channel, int((got != ref).sum()))


def _colorize(cuda, labels, num_classes, want_u8=True):
    lab = torch.from_numpy(labels).to(cuda)
    pal = torch.from_numpy(IC.palette_for(num_classes)).to(cuda).contiguous()
    vis = torch.full(labels.shape + (3,), 99, dtype=torch.uint8, device=cuda)
    lab8 = torch.full(labels.shape, 99, dtype=torch.uint8, device=cuda) if want_u8 else None
    _lib.call("mgu_colorize_labels", cuda, lab, lab.numel(), pal, num_classes, vis, lab8)
    return vis.cpu().numpy(), (lab8.cpu().numpy() if want_u8 else None)


@pytest.mark.parametrize("num_classes", [1, 3, 4, 256])
def test_colour_map_outside_labels_are_black_and_the_label_byte_wraps(cuda, num_classes):
    base = np.array([-1, 0, num_classes - 1, num_classes, num_classes + 1, 255, 256, 257, 300, 511, -256, 2 ** 40 + 1, -2 ** 40], np.int64)
    labels = np.concatenate([base, np.arange(-3, 700)]).reshape(-1, 4)
    vis, lab8 = _colorize(cuda, labels, num_classes)
    ref_vis, ref_u8 = IC.colorize_reference(labels, num_classes, IC.palette_for(num_classes))
    assert np.array_equal(vis, ref_vis) and np.array_equal(lab8, ref_u8)
    flat = vis.reshape(-1, 3)
    assert flat[0].tolist() == [0, 0, 0] and flat[3].tolist() == [0, 0, 0] and flat[2].tolist() == IC.palette_for(num_classes)[-1].tolist()
    if num_classes == 256:
        assert flat[5].tolist() == IC.palette_for(256)[255].tolist() and flat[6].tolist() == [0, 0, 0]
    vis2, none = _colorize(cuda, labels, num_classes, want_u8=False)                # without the label map
    assert none is None and np.array_equal(vis2, ref_vis)
    got_l, got_v = mgunet.postprocess_segmentation(torch.from_numpy(labels).to(cuda), num_classes,
                                                   colors=[tuple(int(v) for v in r) for r in IC.palette_for(num_classes)])
    assert np.array_equal(got_l, labels) and np.array_equal(got_v, ref_vis)


def test_colour_map_of_zero_pixels_writes_nothing(cuda):
    lab = torch.zeros(4, dtype=torch.int64, device=cuda)
    pal = torch.from_numpy(IC.palette_for(3)).to(cuda)
    vis = torch.full((4, 3), 7, dtype=torch.uint8, device=cuda)
    lab8 = torch.full((4,), 7, dtype=torch.uint8, device=cuda)
    _lib.call("mgu_colorize_labels", cuda, lab, 0, pal, 3, vis, lab8)
    assert int(vis.min()) == 7 and int(lab8.min()) == 7


@pytest.mark.parametrize("D,ld,c_off", [(4, 4, 0), (12, 12, 0), (4, 16, 8), (12, 20, 4)])
@pytest.mark.parametrize("R", [0, 1, 7])
def test_region_map_gather(cuda, R, D, ld, c_off):
    table = O.formula_normal("imageio/table", (max(R, 1), D), seed=R + D).astype(np.float32)
    ids = (np.arange(-2, 3 * 67 - 2).reshape(3, 67) % (R + 3)) - 1                   # -1 .. R + 1: both outside ends, every row of the table
    ids[1, 5], ids[2, 9] = -2 ** 40, 2 ** 40
    assert ids.min() < 0 and (ids == -1).any() and (ids == R).any() and (R == 0 or (ids == R - 1).any())
    ref = IC.gather_reference(table[:R], ids)
    out = torch.full(ids.shape + (ld,), float("nan"), device=cuda)
    _lib.call("mgu_region_map_gather_nhwc", cuda, torch.from_numpy(table).to(cuda), R, D, torch.from_numpy(ids).to(cuda), ids.size, out, ld, c_off)
    got = out.cpu().numpy()
    assert np.array_equal(got[..., c_off:c_off + D], ref)
    rest = np.delete(got, np.s_[c_off:c_off + D], axis=-1)
    assert rest.size == ids.size * (ld - D) and np.isnan(rest).all()
    if R == 0:
        assert not got[..., c_off:c_off + D].any()


def test_feature_fusion_gathers_through_the_mirror(cuda):
    fu = torch.from_numpy(O.formula_normal("imageio/fu", (2, 8, 6, 10), seed=3)).to(cuda)
    fg = torch.from_numpy(O.formula_normal("imageio/fg", (5, 12), seed=4)).to(cuda)
    ids = torch.from_numpy((np.arange(120).reshape(2, 6, 10) % 8) - 1).to(cuda)     # -1 .. 6 over R = 5
    got = mgunet.FeatureFusion([8], 12)([fu], fg, region_to_pixel_map=ids)
    ref = O.feature_fusion_full([fu.cpu()], fg.cpu(), 12, region_to_pixel_map=ids.cpu())
    assert torch.equal(got.cpu(), ref)


# ---- 6. fp32 bilinear resize -----------------------------------------------------------------------------------------------------------------------
def _resize(cuda, x, Ho, Wo, mode):
    """mode 'ld_in': the input is a channel slice of a wider NaN-filled buffer; 'c_off': the output is one -> (got, the other channels)"""
    B, Hi, Wi, Cc = x.shape
    xd = torch.from_numpy(x).to(cuda)
    if mode == "ld_in":
        wide = torch.full((B, Hi, Wi, Cc + 8), float("nan"), device=cuda)
        wide[..., 4:4 + Cc] = xd
        src, ld_in, ld_out, c_off = wide[..., 4:4 + Cc], Cc + 8, Cc, 0
    else:
        src, ld_in, ld_out, c_off = xd, Cc, Cc + 12, 8
    out = torch.full((B, Ho, Wo, ld_out), float("nan"), device=cuda)
    _lib.call("mgu_resize_bilinear_nhwc", cuda, src, ld_in, B, Hi, Wi, Cc, out, ld_out, c_off, Ho, Wo)
    o = out.cpu().numpy()
    return o[..., c_off:c_off + Cc].astype(np.float64), np.delete(o, np.s_[c_off:c_off + Cc], axis=-1)


@pytest.mark.parametrize("mode", ["ld_in", "c_off"])
@pytest.mark.parametrize("shape", IC.RESIZE_SHAPES)
def test_resize_bilinear_against_float64(cuda, shape, mode):
    B, Hi, Wi, Ho, Wo, Cc = shape
    x = IC.resize_input(B, Hi, Wi, Cc)
    ref, bar, lo, hi = IC.resize_reference(x, Ho, Wo)
    got, rest = _resize(cuda, x, Ho, Wo, mode)
    assert np.isnan(rest).all() and rest.size == B * Ho * Wo * (0 if mode == "ld_in" else 12)
    err = np.abs(got - ref)
    over = err > bar
    print(f"resize {shape} {mode}: max err {err.max():.3e}  max err/bar {float((err / np.maximum(bar, 1e-300)).max()):.3f}  over {int(over.sum())}"
          f"  below min {int((got < lo).sum())}  above max {int((got > hi).sum())}")
    assert np.isfinite(got).all() and not over.any()
    assert np.all(got >= lo) and np.all(got <= hi)                                  # inside the four sources
    if (Hi, Wi) == (Ho, Wo):
        assert np.array_equal(got, x.astype(np.float64))                            # equal sizes: the input, exactly


def test_resize_two_times_upsampling_of_integers_is_exact(cuda):
    x = IC.resize_input(1, 12, 20, 16, integers=True)
    ref, _, _, _ = IC.resize_reference(x, 24, 40)
    for mode in ("ld_in", "c_off"):
        got, _ = _resize(cuda, x, 24, 40, mode)
        assert np.array_equal(got, ref), mode                                       # weights 1/4 and 3/4 on small integers


def test_resize_through_feature_fusion(cuda):
    """the mirror's own call (ld_in = C, the fused tensor as the wide output) on the two directions"""
    fu0 = torch.from_numpy(IC.resize_input(2, 24, 40, 8)).permute(0, 3, 1, 2).contiguous()
    fu1 = torch.from_numpy(IC.resize_input(2, 7, 9, 4)).permute(0, 3, 1, 2).contiguous()
    fg = torch.from_numpy(IC.resize_input(2, 33, 17, 12)).permute(0, 3, 1, 2).contiguous()
    got = mgunet.FeatureFusion([8, 4], 12)([fu0.to(cuda), fu1.to(cuda)], fg.to(cuda)).cpu().permute(0, 2, 3, 1).numpy().astype(np.float64)
    assert np.array_equal(got[..., :8], fu0.permute(0, 2, 3, 1).numpy().astype(np.float64))
    for sl, src in ((slice(8, 12), fu1), (slice(12, 24), fg)):
        ref, bar, _, _ = IC.resize_reference(src.permute(0, 2, 3, 1).numpy(), 24, 40)
        assert np.all(np.abs(got[..., sl] - ref) <= bar)
