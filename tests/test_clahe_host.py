"""CLAHE without a GPU: the numpy oracle of tests/clahe_oracle.py against an independent per-pixel loop written from the definition
(include/mgunet.h, mgu_clahe_u8), the properties every table has, OpenCV's geometry rule, each branch of the redistribution on tiles
whose tables can be worked out by hand, a fused multiply-add variant that the GPU cases must be able to tell from the definition, the
header's declarations and the argument checks that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import clahe_oracle as O
import mgunet
from mgunet import CLAHE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the loop reference: scalars only, OpenCV's redistribution loop as it is written there ------------------------------------------------
def loop_hist_after_clip(h, clip_limit, area):
    h = [int(v) for v in h]
    if clip_limit > 0:
        cl = max(1, int(clip_limit * area / 256))
        clipped = 0
        for i in range(256):
            if h[i] > cl:
                clipped += h[i] - cl
                h[i] = cl
        batch = clipped // 256
        residual = clipped - batch * 256
        for i in range(256):
            h[i] += batch
        if residual > 0:
            step = max(256 // residual, 1)
            i = 0
            while i < 256 and residual > 0:
                h[i] += 1
                i += step
                residual -= 1
            assert residual == 0                             # every increment lands below 256
    return h


def loop_clahe(img, gy, gx, clip_limit):
    """img (H, W, 1 | 3) uint8 -> (out, tables (gy, gx, 256), histograms after the redistribution (gy, gx, 256))"""
    H, W, ch = img.shape
    if H % gy == 0 and W % gx == 0:
        He, We = H, W
    else:
        He, We = H + gy - H % gy, W + gx - W % gx
    th, tw = He // gy, We // gx
    area = th * tw

    def yuv(p):
        r, g, b = int(p[0]), int(p[1]), int(p[2])
        Y = (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14
        U = min(255, max(0, ((b - Y) * 8061 + (128 << 14) + 8192) >> 14))
        V = min(255, max(0, ((r - Y) * 14369 + (128 << 14) + 8192) >> 14))
        return Y, U, V

    def plane(y, x):
        return int(img[y, x, 0]) if ch == 1 else yuv(img[y, x])[0]

    luts = np.zeros((gy, gx, 256), np.uint8)
    hists = np.zeros((gy, gx, 256), np.int64)
    scale = F(255.0) / F(area)
    for ty in range(gy):
        for tx in range(gx):
            h = [0] * 256
            for y in range(ty * th, ty * th + th):
                for x in range(tx * tw, tx * tw + tw):
                    h[plane(O.reflect(y, H), O.reflect(x, W))] += 1
            h = loop_hist_after_clip(h, clip_limit, area)
            hists[ty, tx] = h
            s = 0
            for i in range(256):
                s += h[i]
                luts[ty, tx, i] = min(255, max(0, int(np.rint(F(np.int32(s)) * scale))))
    out = np.zeros_like(img)
    inv_tw, inv_th = F(1.0) / F(tw), F(1.0) / F(th)
    for y in range(H):
        tyf = F(y) * inv_th - F(0.5)
        ty1 = int(np.floor(tyf))
        ya = tyf - F(ty1)
        ya1 = F(1.0) - ya
        ty2, ty1 = min(ty1 + 1, gy - 1), max(ty1, 0)
        for x in range(W):
            txf = F(x) * inv_tw - F(0.5)
            tx1 = int(np.floor(txf))
            xa = txf - F(tx1)
            xa1 = F(1.0) - xa
            tx2, tx1 = min(tx1 + 1, gx - 1), max(tx1, 0)
            v = plane(y, x)
            top = F(luts[ty1, tx1, v]) * xa1 + F(luts[ty1, tx2, v]) * xa
            bot = F(luts[ty2, tx1, v]) * xa1 + F(luts[ty2, tx2, v]) * xa
            res = top * ya1 + bot * ya
            assert all(type(t) is F for t in (txf, xa, xa1, top, bot, res))
            o = min(255, max(0, int(np.rint(res))))
            if ch == 1:
                out[y, x, 0] = o
            else:
                _, U, V = yuv(img[y, x])
                u, w = U - 128, V - 128
                rgb = (o + ((w * 18678 + 8192) >> 14), o + ((u * -6472 + w * -9519 + 8192) >> 14), o + ((u * 33292 + 8192) >> 14))
                out[y, x] = [min(255, max(0, c)) for c in rgb]
    return out, luts, hists


LOOP_CASES = [(1, 1, 1, 1), (3, 5, 8, 8), (13, 9, 3, 2), (1, 1, 8, 8)]       # H, W, grid_y, grid_x


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("clip", [0.0, 0.01, 2.0, 40.0])
@pytest.mark.parametrize("H,W,gy,gx", LOOP_CASES)
def test_the_oracle_equals_the_loop_reference_and_the_tables_have_their_properties(H, W, gy, gx, clip, ch):
    img = np.random.RandomState(H * 100 + W + ch).randint(0, 256, (H, W, ch)).astype(np.uint8)
    want, wluts, hists = loop_clahe(img, gy, gx, clip)
    got, luts = O.clahe(img[None], gy, gx, clip)
    assert np.array_equal(luts[0], wluts) and np.array_equal(got[0], want)
    _he, _we, th, tw = O.geometry(H, W, gy, gx)
    v = img[None, :, :, 0].astype(np.int64) if ch == 1 else O.rgb2yuv(img[None])[0]
    h = O.redistribute(O.histograms(v, gy, gx), O.clip_value(clip, th * tw))
    assert np.array_equal(h[0], hists)
    assert bool((h.sum(-1) == th * tw).all()) and bool((h >= 0).all())                       # the counts of a tile add up to its area
    assert bool((np.diff(luts.astype(np.int64), axis=-1) >= 0).all()) and bool((luts[..., 255] == 255).all())


@pytest.mark.parametrize("H,W,gy,gx,clip", [(65, 129, 4, 3, 4.0), (50, 70, 8, 8, 2.0), (130, 70, 2, 64, 40.0), (64, 60, 8, 8, 0.01)])
def test_table_properties_on_the_larger_cases(H, W, gy, gx, clip):
    img = np.random.RandomState(H + W).randint(0, 256, (2, H, W, 1)).astype(np.uint8)
    img[1] = img[1] // 8 + 100                                                                  # a flat image: most of it is clipped
    _he, _we, th, tw = O.geometry(H, W, gy, gx)
    h = O.redistribute(O.histograms(img[..., 0].astype(np.int64), gy, gx), O.clip_value(clip, th * tw))
    assert bool((h.sum(-1) == th * tw).all())
    out, luts = O.clahe(img, gy, gx, clip)
    assert out.shape == img.shape and out.dtype == np.uint8
    assert bool((np.diff(luts.astype(np.int64), axis=-1) >= 0).all()) and bool((luts[..., 255] == 255).all())


def test_one_tile_without_a_clip_is_a_plain_table_lookup():
    img = np.random.RandomState(3).randint(0, 256, (1, 40, 24, 1)).astype(np.uint8)
    out, luts = O.clahe(img, 1, 1, 0.0)
    assert np.array_equal(out[0, :, :, 0], luts[0, 0, 0][img[0, :, :, 0]])
    hist = np.bincount(img.reshape(-1), minlength=256)
    assert np.array_equal(luts[0, 0, 0], np.rint(np.cumsum(hist) * 255.0 / 960.0).astype(np.uint8))     # no product is near a tie here


def test_geometry_is_opencvs():
    assert O.geometry(64, 60, 8, 8) == (72, 64, 9, 8)       # the axis that divides is extended by a whole grid as well
    assert O.geometry(64, 64, 8, 8) == (64, 64, 8, 8)
    assert O.geometry(3, 5, 8, 8) == (8, 8, 1, 1)
    assert O.geometry(130, 70, 2, 64) == (132, 128, 66, 2)
    assert [O.reflect(i, 3) for i in range(-5, 8)] == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert [O.reflect(i, 1) for i in (-2, 0, 5)] == [0, 0, 0]


def by_hand(side, clip_limit, value=77):
    """the table of one side x side tile of a constant value from the closed form, in exact integer arithmetic -> (lut, batch,
    residual, step); no S * 255 / area of these cases lies within 1e-4 of a tie, so neither the rounding mode nor fp32 matters"""
    area = side * side
    cl = max(1, int(clip_limit * area / 256))
    clipped = max(area - cl, 0)
    batch, residual = divmod(clipped, 256)
    step = max(256 // residual, 1) if residual else 0
    h = [batch] * 256
    h[value] += min(area, cl)
    for k in range(residual):
        h[k * step] += 1
    assert sum(h) == area
    lut, s = [], 0
    for i in range(256):
        s += h[i]
        r = s * 255 % area
        assert abs(2 * r - area) * 10000 > 2 * area, (i, s)          # |fraction - 1/2| > 1e-4: fp32's 255 * 2^-23 cannot cross the tie
        lut.append((2 * s * 255 + area) // (2 * area))
    return np.array(lut, np.uint8), batch, residual, step


REDISTRIBUTION = [(16, 255.0, (0, 1, 256), [1, 1, 255, 255, 255]), (16, 128.0, (0, 128, 2), [1, 39, 166, 192, 255]),
                  (16, 100.0, (0, 156, 1), [1, 77, 177, 228, 255]), (32, 64.0, (3, 0, 0), None)]


@pytest.mark.parametrize("side,clip,branch,probe", REDISTRIBUTION)
def test_every_branch_of_the_redistribution(side, clip, branch, probe):
    lut, batch, residual, step = by_hand(side, clip)
    assert (batch, residual, step) == branch
    if probe is not None:
        assert lut[[0, 76, 77, 128, 255]].tolist() == probe
    img = np.full((1, side, side, 1), 77, np.uint8)
    out, luts = O.clahe(img, 1, 1, clip)
    assert np.array_equal(luts[0, 0, 0], lut)
    assert bool((out == lut[77]).all())
    assert np.array_equal(loop_clahe(img[0], 1, 1, clip)[1][0, 0], lut)


def test_a_fused_multiply_add_is_seen_where_the_tile_side_is_no_power_of_two():
    """what a compiler that contracts a * b + c would compute differs from the definition on the GPU tests' cases with 12 x 12 and
    7 x 9 tiles, and not with 16 x 16 tiles, where every product is exact"""
    for H, W, clip, seed, differs in ((96, 96, 0.0, 11, True), (50, 70, 2.0, 12, True), (128, 128, 2.0, 13, False)):
        img = np.random.RandomState(seed).randint(0, 256, (1, H, W, 1)).astype(np.uint8)
        plain, luts = O.clahe(img, 8, 8, clip)
        fused, luts_f = O.clahe(img, 8, 8, clip, fused=True)
        assert np.array_equal(luts, luts_f)
        n = int((plain != fused).sum())
        print(f"fused variant at {H} x {W}, clip {clip}: {n} bytes differ")
        assert (n > 0) == differs, (H, W, n)
        assert int(np.abs(plain.astype(int) - fused.astype(int)).max()) <= 1


def test_names_are_exported_and_declared():
    for name in ("CLAHE", "patch_clahe_features_u8"):
        assert name in mgunet.__all__ and callable(getattr(mgunet, name)), name
    assert callable(mgunet.HistogramEqualizer.clahe_rgb) and callable(mgunet.HistogramEqualizer.clahe_gray)
    header = open(os.path.join(ROOT, "include", "mgunet.h")).read()
    for name in ("mgu_clahe_u8", "mgu_patch_clahe_mean_u8"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    protos = mgunet._lib.parse_header()
    a, b = protos["mgu_clahe_u8"], protos["mgu_patch_clahe_mean_u8"]
    assert a[2] and b[2]                                                     # both end in hip_stream
    assert len(a[1]) == 12 and a[1][8] is ctypes.c_double and a[1][2:8] == [ctypes.c_int] * 6 and a[1][9:11] == [ctypes.c_void_p] * 2
    assert len(b[1]) == 14 and b[1][8] is ctypes.c_double and b[1][2:8] == [ctypes.c_int] * 6 and b[1][9] is ctypes.c_int
    assert b[1][10] is ctypes.c_void_p and b[1][11:13] == [ctypes.c_int] * 2
    mk = open(os.path.join(ROOT, "mingraph-unet_amd", "csrc", "Makefile")).read()
    assert "clahe.hip" in mk and os.path.exists(os.path.join(ROOT, "mingraph-unet_amd", "csrc", "clahe.hip"))
    section = " ".join(header[header.index("Contrast-limited adaptive"):header.index("int mgu_clahe_u8")].replace("*", " ").split())
    assert "NOT verified" in section and "no fused multiply-add" in section and "72 x 64" in section


def test_argument_checks_that_need_no_device():
    c = CLAHE()
    assert c.clip_limit == 40.0 and c.tile_grid_size == (8, 8)
    assert CLAHE(2, (3, 4)).grid_yx == (4, 3)                                # tile_grid_size is (x, y), as cv2's
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="clip_limit"):
            CLAHE(bad)
    for bad in ((0, 8), (8, 0), (65, 8), (8, 65), (8,), (8, 8, 8), (2.5, 8), 8, None):
        with pytest.raises(ValueError, match="tile_grid_size"):
            CLAHE(2.0, bad)
    with pytest.raises(TypeError, match="uint8"):
        c.apply(np.zeros((4, 4), np.float32))
    with pytest.raises(TypeError, match="uint8"):
        c.apply(torch.zeros(4, 4))
    with pytest.raises(TypeError):
        c.apply([[1, 2], [3, 4]])
    for shape, ch in (((4, 4, 5), None), ((2, 4, 4), None), ((4,), None), ((2, 4, 4, 2), None), ((4, 4), 3), ((2, 4, 4, 1), 3),
                      ((4, 4), 2), ((0, 4), None), ((2, 0, 4, 3), None), ((1, 2, 3, 4, 3), None)):
        with pytest.raises(ValueError):
            c.apply(np.zeros(shape, np.uint8), channels=ch)
        with pytest.raises(ValueError):
            c.tables(torch.zeros(shape, dtype=torch.uint8), channels=ch)
    assert CLAHE._batch_shape(np.zeros((2, 4, 5), np.uint8), 1) == (2, 4, 5, 1)
    assert CLAHE._batch_shape(np.zeros((4, 5, 3), np.uint8), 1) == (4, 5, 3, 1)       # stated: four grey images, not one RGB image
    assert CLAHE._batch_shape(np.zeros((4, 5, 1), np.uint8), None) == (1, 4, 5, 1)
    assert CLAHE._batch_shape(torch.zeros((4, 5, 3), dtype=torch.uint8), 3) == (1, 4, 5, 3)
    with pytest.raises(ValueError, match="out"):
        c.apply(np.zeros((4, 4), np.uint8), out=np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError, match="out"):
        c.apply(np.zeros((4, 4), np.uint8), out=torch.zeros((4, 4), dtype=torch.uint8))
    eq = mgunet.HistogramEqualizer()
    with pytest.raises(ValueError, match="RGB"):
        eq.clahe_rgb(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match="grey"):
        eq.clahe_gray(np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="tile_grid_size"):
        eq.clahe_rgb(np.zeros((4, 4, 3), np.uint8), tile_grid_size=(0, 1))
    with pytest.raises(TypeError, match="CLAHE"):
        mgunet.patch_clahe_features_u8(np.zeros((4, 4, 3), np.uint8), 2, mgunet.GaussianSmoother())
    with pytest.raises(TypeError, match="CLAHE"):
        mgunet.patch_node_features(np.zeros((4, 4, 3), np.uint8), 2, equalizer=mgunet.HistogramEqualizer())
