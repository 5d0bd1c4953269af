"""The cases of tests/image_io_cases.py on the CPU: each reference against its independent counterpart (PIL itself, scipy's Sobel, the
exact integer normalisation, F.interpolate), each adversarial case's property with its count, and each named wrong variant shown to
differ from the reference on at least one case that tests/test_gpu_image_io.py runs.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_io_cases as IC
import mgunet_oracle as O


# ---- 1. PIL resample ------------------------------------------------------------------------------------------------------------------------
def _resample_inputs():
    for src, dst in IC.RESAMPLE_PAIRS:
        for content in IC.RESAMPLE_CONTENTS:
            for layout in ("rgb", "grey"):
                yield src, dst, content, layout, IC.resample_image(content, src, layout)


def test_resample_restatement_is_pil():
    """the restatement that carries the variants equals real PIL on every case, and PIL keeps all-255 at 255"""
    n = 0
    for src, dst, content, layout, img in _resample_inputs():
        ref = IC.pil_resize_u8(img, dst)
        assert np.array_equal(IC.pil_resample(img, dst), ref), (src, dst, content, layout)
        if content == "full":
            assert int(ref.min()) == 255, (src, dst)
        n += 1
    assert n == 9 * 5 * 2


def test_resample_cases_have_their_properties():
    def taps(s, d):
        return [c for _, c in IC.pil_coeffs(s, d)[0]]
    # (2,3) -> (64,64): support 1, two taps inside, ONE where the window is clipped at a border: 22 and 32 of the 64 outputs
    assert sum(c == 1 for c in taps(3, 64)) == 22 and sum(c == 2 for c in taps(3, 64)) == 42
    assert sum(c == 1 for c in taps(2, 64)) == 32 and sum(c == 2 for c in taps(2, 64)) == 32          # two taps = the whole column
    assert taps(7, 1) == [7] and taps(5, 1) == [5] and taps(1, 7) == [1] * 7                         # the window is the whole row
    assert taps(1080, 2) == [810, 810] and taps(300, 4) == [113, 150, 150, 112]                      # hundreds of taps, clipped outside
    assert taps(3, 2) == [2, 2]
    for (src, dst) in IC.RESAMPLE_PAIRS:                            # which passes run
        h, v = src[1] != dst[1], src[0] != dst[0]
        assert (h, v) == {((5, 5), (5, 9)): (True, False), ((9, 5), (5, 5)): (False, True), ((64, 64), (64, 64)): (False, False)}.get((src, dst), (True, True))
    tall = [(src, dst) for src, dst in IC.RESAMPLE_PAIRS if src[0] > 100 * src[1] and dst[0] < src[0] and src[1] != dst[1]]
    assert tall == [((1080, 3), (2, 2))]                            # the one pair Image.resize takes vertical pass first


def _differs_from_pil(variant):
    hits = []
    for src, dst, content, layout, img in _resample_inputs():
        if not np.array_equal(IC.pil_resample(img, dst, variant), IC.pil_resize_u8(img, dst)):
            hits.append((src, dst, content, layout))
    return hits


@pytest.mark.parametrize("variant", ["vertical_first", "horizontal_always", "no_round_window", "no_half"])
def test_resample_wrong_variants_differ_from_pil(variant):
    hits = _differs_from_pil(variant)
    print(variant, len(hits), hits[:4])
    assert hits, variant
    if variant == "horizontal_always":
        assert {h[:2] for h in hits} == {((1080, 3), (2, 2))}


def test_resample_window_start_without_rounding_is_the_same_function():
    """floor(center - support) never starts later than int(center - support + 0.5), and the taps it adds lie outside the triangle's
    support: weight zero.  Asserted on every table of the suite; no case can tell it from PIL."""
    for src, dst in IC.RESAMPLE_PAIRS:
        for s, d in zip(src, dst):
            (b0, r0), (b1, r1) = IC.pil_coeffs(s, d), IC.pil_coeffs(s, d, "floor_start")
            for (f0, c0), k0, (f1, c1), k1 in zip(b0, r0, b1, r1):
                assert f1 <= f0 and f1 + c1 == f0 + c0 and k1[:f0 - f1] == [0] * (f0 - f1) and k1[f0 - f1:] == k0
    assert _differs_from_pil("floor_start") == []


def test_resample_sign_blind_rounding_cannot_differ_for_the_triangle_filter():
    """`+0.5 regardless of sign` differs from PIL only where a coefficient is negative.  BILINEAR's triangle never is (asserted over every
    table of the suite), so no case of this kernel can tell the two apart; the variant is real, though: on a BICUBIC resize, whose
    filter has negative lobes, it departs from PIL while the restatement with PIL's rule does not."""
    for src, dst in IC.RESAMPLE_PAIRS:
        for s, d in zip(src, dst):
            assert min(min(r) for r in IC.pil_coeffs(s, d)[1]) >= 0
    assert _differs_from_pil("round_plus_half") == []
    img = np.random.RandomState(3).randint(0, 256, (200, 200, 3)).astype(np.uint8)
    ref = IC.pil_resize_u8(img, (64, 64), "bicubic")
    assert min(min(r) for r in IC.pil_coeffs(200, 64, filt="bicubic")[1]) < 0
    assert np.array_equal(IC.pil_resample(img, (64, 64), None, "bicubic"), ref)
    assert int((IC.pil_resample(img, (64, 64), "round_plus_half", "bicubic") != ref).sum()) == 4


# ---- 2. mask resize -------------------------------------------------------------------------------------------------------------------------
def test_mask_reference_is_the_double_index_rule():
    for src, dst in IC.MASK_PAIRS:
        m = IC.mask_image(src)
        for nc in IC.MASK_CLASSES:
            assert np.array_equal(O.preprocess_mask(m, dst, nc).numpy(), IC.mask_variant(m, dst, nc)), (src, dst, nc)
    m = IC.mask_image((539, 77))
    assert np.array_equal(np.unique(m), np.arange(256))               # the clip is reached at both ends for every class count
    assert int(O.preprocess_mask(m, (693, 99), 3).max()) == 2 and int(O.preprocess_mask(m, (693, 99), 1).max()) == 0
    assert int(O.preprocess_mask(m, (693, 99), 256).max()) == 255


def test_mask_cases_where_the_arithmetic_decides():
    def n_diff(s, d, variant):
        return int((IC.mask_index(s, d) != IC.mask_index(s, d, variant)).sum())
    assert n_diff(539, 693, "exact") == 76 and n_diff(539, 693, "float32") == 76
    assert np.array_equal(IC.mask_index(539, 693, "exact") != IC.mask_index(539, 693), IC.mask_index(539, 693, "float32") != IC.mask_index(539, 693))
    got = {(s, d): n_diff(s, d, "exact") for s, d in ((77, 99), (21, 27), (42, 54), (6, 34))}
    print(got)
    assert got[(6, 34)] == 1 and all(got[k] > 0 for k in ((77, 99), (21, 27), (42, 54)))
    for s, d in ((100, 300), (300, 100), (1, 9), (13, 1), (31, 31)):
        assert n_diff(s, d, "exact") == 0, (s, d)
    # the double rule lands one BELOW the exact index wherever it differs: floor(x * (1 / (9/7))) just under an integer
    idx = IC.mask_index(539, 693)
    assert np.all((IC.mask_index(539, 693, "exact") - idx)[idx != IC.mask_index(539, 693, "exact")] == 1)


@pytest.mark.parametrize("variant", IC.MASK_VARIANTS)
def test_mask_wrong_variants_differ(variant):
    m = IC.mask_image((539, 77))
    ref = O.preprocess_mask(m, (693, 99), 256).numpy()
    assert not np.array_equal(IC.mask_variant(m, (693, 99), 256, variant), ref)
    m = IC.mask_image((21, 42))                                       # the smaller member, on the other axis
    assert not np.array_equal(IC.mask_variant(m, (27, 54), 256, variant), O.preprocess_mask(m, (27, 54), 256).numpy())


# ---- 3. Sobel -------------------------------------------------------------------------------------------------------------------------------
def _scipy_mag2(rgb):
    from scipy import ndimage
    g = IC.cv_gray(rgb).astype(np.int64)
    gx, gy = ndimage.sobel(g, axis=1, mode="mirror"), ndimage.sobel(g, axis=0, mode="mirror")
    return gx * gx + gy * gy


def test_sobel_reference_is_scipy_and_the_exact_rule():
    for name, img in IC.sobel_cases().items():
        ref = O.sobel_edges(img)
        m = _scipy_mag2(img)
        assert np.array_equal(m, IC.sobel_mag2(img)), name
        if m.max() > 0:
            mag = np.sqrt(m.astype(np.float64))
            assert np.array_equal((mag / mag.max() * 255).astype(np.uint8), ref), name
        else:
            assert int(ref.max()) == 0, name
        assert np.array_equal(IC.sobel_exact(img), ref), name
        assert np.array_equal(IC.sobel_variant(img), ref), name
    assert {"noise_1x1", "noise_1x9", "noise_9x1", "noise_2x2", "noise_2x7", "noise_3x3", "noise_37x45"} <= set(IC.sobel_cases())


def test_sobel_tie_dense_is_integer_valued_at_every_pixel():
    img = IC.tie_dense()
    assert img.shape == (8, 1539, 3) and img.shape[0] * img.shape[1] == 12312
    m = IC.sobel_mag2(img)
    M = int(m.max())
    assert M == 1020 * 1020
    k = np.sqrt(m.astype(np.float64)).astype(np.int64) // 4
    assert np.array_equal(16 * k * k, m)                              # every gradient is 4k
    assert int((k * k * M == 65025 * m).sum()) == 12312               # 255 sqrt(m / M) = k exactly, at all 12312 pixels
    ref = O.sobel_edges(img)
    assert np.array_equal(ref, k.astype(np.uint8)) and np.array_equal(ref, IC.sobel_exact(img))
    assert np.array_equal(np.unique(ref), np.arange(256))             # every k occurs: one ulp low anywhere shows


def test_sobel_case_properties():
    c = IC.sobel_cases()
    assert int((IC.sobel_mag2(c["single_gradient"]) > 0).sum()) == 1 and int(O.sobel_edges(c["single_gradient"])[1, 0]) == 255
    for name in ("flat_0", "flat_255", "flat_colour"):
        assert int(IC.sobel_mag2(c[name]).max()) == 0
    # last_block: 32 blocks of 256 pixels; every block sees a gradient, the largest lies in the last block alone
    H, W = IC.SOBEL_BLOCK_SHAPE
    assert H * W == 256 * 8 * 4
    per_block = IC.sobel_mag2(c["last_block"]).reshape(-1, 256).max(axis=1)
    assert per_block.size == 32 and per_block.min() > 0 and per_block.argmax() == 31 and np.sort(per_block)[-2] < per_block[31]
    g = IC.cv_gray(IC.colour_cube())
    assert IC.colour_cube().shape == (52, 2704, 3) and np.array_equal(np.unique(g), np.arange(256))
    assert int((g != IC.cv_gray(IC.colour_cube(), 14)).sum()) > 0


@pytest.mark.parametrize("variant", IC.SOBEL_VARIANTS)
def test_sobel_wrong_variants_differ(variant):
    hits = [n for n, img in IC.sobel_cases().items() if not np.array_equal(IC.sobel_variant(img, variant), O.sobel_edges(img))]
    print(variant, hits)
    assert hits, variant
    if variant == "float32":      # correctly rounded float32 division lands on the integer at every exact tie, as float64 does: tie_dense
        assert "near_tie" in hits and "tie_dense" not in hits         # catches a division or root that is NOT correctly rounded


# ---- 4. histogram equalisation ----------------------------------------------------------------------------------------------------------------
def test_equalize_restatement_is_the_oracle():
    for name, img in IC.histeq_cases().items():
        assert np.array_equal(IC.equalize_variant(img), O.equalize_histogram_rgb(img)), name


def test_cube_hits_both_clips_of_v_and_u_cannot_saturate():
    Y, U, V = IC.yuv_preclip(IC.colour_cube())
    n = {"v_low": int((V < 0).sum()), "v_high": int((V > 255).sum()), "u_low": int((U < 0).sum()), "u_high": int((U > 255).sum())}
    print(n, int(U.min()), int(U.max()), int(V.min()), int(V.max()))
    assert n["v_low"] > 0 and n["v_high"] > 0
    red = np.array([[[255, 0, 0]]], np.uint8)
    assert int(IC.yuv_preclip(red)[0][0, 0]) == 76 and int(IC.yuv_preclip(red)[2][0, 0]) == 285
    # U = 128 + 0.492 (B - Y): extreme at pure blue / pure yellow, both in the cube; it stays inside [0, 255], so U has no clip to hit
    assert n["u_low"] == 0 and n["u_high"] == 0
    corners = IC.histeq_cases()["corners"][:1]
    Uc = IC.yuv_preclip(corners)[1]
    assert int(Uc.min()) == int(U.min()) > 0 and int(Uc.max()) == int(U.max()) < 255


def test_half_tie_table():
    hist = np.zeros(256, np.int64)
    for lvl, cnt in IC.half_tie_counts().items():
        hist[lvl] = cnt
    assert hist.sum() - hist[0] == 510 and np.float32(255.0) / np.float32(510) == 0.5
    csum = np.cumsum(hist) - hist[0]
    ties = int((csum[1:] % 2 == 1).sum())
    assert ties == 254 and ties >= 100
    lut, up = IC.equalize_table(hist), IC.equalize_table(hist, "half_up")
    assert np.array_equal(lut[1:255], 2 * (np.arange(1, 255) // 2))                # i - 1/2 -> the even neighbour
    assert int((lut != up).sum()) == 127                                           # every tie whose lower neighbour is even
    img = IC.histeq_cases()["half_ties"]
    assert np.array_equal(np.bincount(IC.yuv_preclip(img)[0].reshape(-1), minlength=256), hist)


def test_histeq_case_properties():
    c = IC.histeq_cases()
    def hist(name):
        return np.bincount(IC.yuv_preclip(c[name])[0].reshape(-1), minlength=256)
    assert int((hist("constant") > 0).sum()) == 1 and int((hist("two_levels") > 0).sum()) == 2
    h = hist("all_but_one")
    assert h[17] == h.sum() - 1 and np.array_equal(np.unique(O.equalize_histogram_rgb(c["all_but_one"])), [0, 255])
    h = hist("scale_probe")
    assert h.sum() - h[0] == 210
    a, b = IC.equalize_table(h), IC.equalize_table(h, "scale_double")
    assert int((a != b).sum()) == 6 * 10 and np.array_equal(np.abs(a - b).max(), 1)   # six sums, each held for ten levels
    assert IC.HISTEQ_BIG_SHAPE[0] * IC.HISTEQ_BIG_SHAPE[1] >= 1024 * 256 * 8


@pytest.mark.parametrize("variant", IC.HISTEQ_VARIANTS)
def test_histeq_wrong_variants_differ(variant):
    hits = [n for n, img in IC.histeq_cases().items() if not np.array_equal(IC.equalize_variant(img, variant), O.equalize_histogram_rgb(img))]
    print(variant, hits)
    assert hits, variant
    need = {"half_up": "half_ties", "scale_double": "scale_probe", "uv_unsaturated": "cube", "cumsum_with_i0": "half_ties"}[variant]
    assert need in hits


# ---- 5. patch means, colour map, gather -------------------------------------------------------------------------------------------------------
def test_patch_mean_exact_reference():
    for H, W, C, p in IC.PATCH_MEAN_CASES:
        img = IC.patch_mean_image(H, W, C)
        for pc in (False, True):
            ref = IC.patch_mean_exact(img, p, pc)
            assert ref.shape == (-(-H // p) * -(-W // p), C if pc else 1)
            if p <= 32:                                                # the oracle's fp32 mean: the same value to fp32 summation error
                assert float((ref - O.patch_mean_u8(img, p, pc)).abs().max()) <= 1e-4
    H, W, C, p = IC.PATCH_MEAN_FULL
    assert 2 ** 31 < H * W * C * 255 < 2 ** 32 and p > max(H, W)
    assert float(IC.patch_mean_exact(IC.patch_mean_image(2, 3, 2, full=True), 1, True).min()) == 255.0
    side, C = IC.PATCH_MEAN_WIDE
    assert side * side * C * 255 == 12834570240 > 2 ** 32 and side * side * 255 < 2 ** 32      # one channel's sum still fits


def test_colorize_reference_pins_the_label_byte():
    labels = np.array([[-1, 0, 1, 2, 3, 255, 256, 300, 511, -256]], np.int64)
    vis, lab8 = IC.colorize_reference(labels, 3, IC.palette_for(3))
    assert lab8.tolist() == [[255, 0, 1, 2, 3, 255, 0, 44, 255, 0]]
    assert vis[0, 0].tolist() == [0, 0, 0] and vis[0, 4].tolist() == [0, 0, 0] and vis[0, 3].tolist() == IC.palette_for(3)[2].tolist()
    assert int(IC.palette_for(256).max(axis=1).min()) > 0               # no class is black: black means `outside`


# ---- 6. fp32 bilinear resize --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", IC.RESIZE_SHAPES)
def test_resize_reference_is_aten(shape):
    B, Hi, Wi, Ho, Wo, C = shape
    x = IC.resize_input(B, Hi, Wi, C)
    nchw = torch.from_numpy(x).permute(0, 3, 1, 2)
    # float64 end to end: the same formula, so agreement to a few float64 roundings
    ref64, _, lo, hi = IC.resize_reference(x, Ho, Wo, coord=np.float64)
    at64 = F.interpolate(nchw.double(), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    scale = np.abs(x).max()
    assert np.abs(at64 - ref64).max() <= 8 * 2.0 ** -52 * scale
    assert np.all(ref64 >= lo) and np.all(ref64 <= hi)
    # float32 aten against the float64 blend at the float32 coordinates: inside the bar the kernel is held to
    ref, bar, _, _ = IC.resize_reference(x, Ho, Wo)
    at32 = F.interpolate(nchw, size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy().astype(np.float64)
    ratio = np.abs(at32 - ref) / np.maximum(bar, 1e-300)
    print(shape, "aten fp32 err / bar", float(ratio.max()))
    assert np.all(np.abs(at32 - ref) <= bar)
    if (Hi, Wi) == (Ho, Wo):
        assert np.array_equal(ref, x.astype(np.float64))


def test_resize_two_times_upsampling_of_integers_is_exact():
    x = IC.resize_input(1, 12, 20, 16, integers=True)
    ref, _, _, _ = IC.resize_reference(x, 24, 40)
    assert np.array_equal(ref, ref.astype(np.float32).astype(np.float64)) and np.array_equal(ref * 16, np.rint(ref * 16))
    at = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=(24, 40), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(at.astype(np.float64), ref)
