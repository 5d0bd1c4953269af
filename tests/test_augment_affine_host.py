"""CPU tier of the scale / crop / colour augmentation (RandomAffineColor, mgu_augment_affine_color): the names it adds, the argument
refusals with their messages, the numpy oracle's own properties (exact permutations, the half-pixel blend, the colour identities, both
clamps), the oracle against float64 bilinear on every case, color_matrix_q12 and affine_fixed against float64, the draw order, and
nine wrong readings of the definition that the shared cases tell apart.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import mgunet
import augment_affine_cases as AC
import augment_affine_oracle as AO
from mgunet import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = (65536, 0, 0, 0, 65536, 0)
CID = (4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0)
RNG = np.random.default_rng(11)
LUMA_TILES = -(-8192 * 8192 // int(_lib.lib().mgu_augment_luma_tile()))      # luma workgroups of one 8192 x 8192 source
LUMA_B = -(-2 ** 31 // LUMA_TILES)                                            # the smallest batch of them that no launch takes


def test_names_are_declared_bound_and_exported():
    for name in ("RandomAffineColor", "affine_fixed", "color_matrix_q12"):
        assert name in mgunet.__all__ and callable(getattr(mgunet, name)), name
    header = open(os.path.join(ROOT, "include", "mgunet.h")).read()
    for name in ("mgu_augment_affine_color", "mgu_augment_luma_tile", "mgu_augment_luma_sums"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert hasattr(_lib.lib(), name)
    protos = mgunet._lib.parse_header()
    assert protos["mgu_augment_affine_color"][2] and protos["mgu_augment_luma_sums"][2] and not protos["mgu_augment_luma_tile"][2]
    args = protos["mgu_augment_affine_color"][1]
    assert len(args) == 20 and args[16] is C.c_int64 and args[2:6] == [C.c_int] * 4      # context and stream included; mask_fill is 64 bits
    assert "augment_affine.hip" in open(os.path.join(ROOT, "mingraph-unet_amd", "csrc", "Makefile")).read()
    assert int(_lib.lib().mgu_augment_luma_tile()) >= 256
    for word in ("sx = a2 + y a1 + x a0", "(k m + 128) >> 8", "+ 32768) >> 16", "+ 2048) >> 12"):      # the definition is in the header
        assert word in header, word


def abi_args(**kw):
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    a = dict(img=p, B=1, Hs=16, Ws=16, bgr=0, mask=None, nc=0, out=p, H=16, W=16, st=(C.c_int64 * 4)(768, 256, 16, 1),
             mean=(C.c_float * 3)(0.5, 0.5, 0.5), std=(C.c_float * 3)(0.5, 0.5, 0.5), fill=(C.c_uint8 * 3)(0, 0, 0), mout=None, mfill=-100,
             params=p, need_mean=1)
    for k, v in kw.items():
        a[k] = p if v == "set" else v
    return list(a.values())


@pytest.mark.parametrize("kw, message", [
    (dict(img=None), "null pointer"), (dict(out=None), "null pointer"), (dict(st=None), "null pointer"), (dict(mean=None), "null pointer"),
    (dict(std=None), "null pointer"), (dict(fill=None), "null pointer"), (dict(params=None), "null pointer"),
    (dict(B=0), ">= 1"), (dict(Hs=0), ">= 1"), (dict(Ws=0), ">= 1"), (dict(H=0), ">= 1"), (dict(W=-3), ">= 1"),
    (dict(Hs=8193), "above 8192"), (dict(Ws=8193), "above 8192"), (dict(H=8193), "above 8192"), (dict(W=8193), "above 8192"),
    (dict(mask="set"), "go together"), (dict(mout="set"), "go together"),
    (dict(B=32768, H=8192, W=8192), "2^31"), (dict(B=LUMA_B, Hs=8192, Ws=8192), "2^31"),
    ({}, "null context")])
def test_each_refusal_returns_invalid_with_its_message_before_any_device_work(kw, message):
    L = _lib.lib()
    assert L.mgu_augment_affine_color(None, *abi_args(**kw), None) == _lib.MGU_ERR_INVALID
    assert message in L.mgu_last_error(None).decode(), (kw, L.mgu_last_error(None))


def test_luma_sums_refusals_and_limits_just_inside():
    L = _lib.lib()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    for args, message in (((None, 1, 4, 4, 0, p), "null pointer"), ((p, 1, 4, 4, 0, None), "null pointer"), ((p, 0, 4, 4, 0, p), ">= 1"),
                          ((p, 1, 8193, 4, 0, p), "above 8192"), ((p, LUMA_B, 8192, 8192, 0, p), "2^31"), ((p, 1, 4, 4, 0, p), "null context")):
        assert L.mgu_augment_luma_sums(None, *args, None) == _lib.MGU_ERR_INVALID
        assert message in L.mgu_last_error(None).decode(), args
    # one below each limit passes the argument checks (and stops at the missing context)
    for kw in (dict(Hs=8192, Ws=8192, H=8192, W=8192), dict(B=32767, H=8192, W=8192), dict(B=LUMA_B - 1, Hs=8192, Ws=8192), dict(mask="set", mout="set")):
        assert L.mgu_augment_affine_color(None, *abi_args(**kw), None) == _lib.MGU_ERR_INVALID
        assert "null context" in L.mgu_last_error(None).decode(), kw


def test_cpu_tensors_are_refused():
    aug = mgunet.RandomAffineColor(16)
    with pytest.raises(RuntimeError, match="HIP device"):
        aug(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.preprocess.luma_sums(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        aug(torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError):
        mgunet.RandomAffineColor(16, fill=(0, 0, 256))
    with pytest.raises(ValueError):
        mgunet.RandomAffineColor(16, scale=(2.0, 0.5))


# ---- the oracle's own properties ------------------------------------------------------------------------------------------------------
def run1(img, table, out_hw, mask=None, **kw):
    out, byts, smp, ms = AO.augment(img[None], np.asarray([table]), out_hw, AC.MEAN, AC.STD, masks=None if mask is None else mask[None], **kw)
    return out[0], byts[0], smp[0], (None if ms is None else ms[0])


def test_identity_flip_quarter_turn_and_translation_are_exact_permutations():
    img = RNG.integers(0, 256, (12, 12, 3), dtype=np.uint8)
    mask = RNG.integers(0, 256, (12, 12), dtype=np.uint8)
    out, byts, _, ms = run1(img, IDENT + CID, (12, 12), mask)
    assert np.array_equal(byts, img) and np.array_equal(ms, mask.astype(np.int64))
    assert np.array_equal(out, AO.normalize(img.astype(np.int64), AC.MEAN, AC.STD))
    assert mgunet.affine_fixed(0, 0.0, 1.0, 1.0, 0.3, -0.4, (12, 12), (12, 12)) == IDENT
    _, byts, _, ms = run1(img, mgunet.affine_fixed(1, 0.0, 1.0, 1.0, 0, 0, (12, 12), (12, 12)) + CID, (12, 12), mask)
    assert np.array_equal(byts, img[:, ::-1]) and np.array_equal(ms, mask[:, ::-1].astype(np.int64))
    _, byts, _, ms = run1(img, mgunet.affine_fixed(0, 90.0, 1.0, 1.0, 0, 0, (12, 12), (12, 12)) + CID, (12, 12), mask)
    assert np.array_equal(byts, np.rot90(img)) and np.array_equal(ms, np.rot90(mask).astype(np.int64))      # counter-clockwise, as PIL's rotate
    # output (x, y) reads source (x + 3, y - 2): fill where that lies outside
    _, byts, _, ms = run1(img, (65536, 0, 3 * 65536, 0, 65536, -2 * 65536) + CID, (12, 12), mask, fill=(9, 8, 7), mask_fill=-100)
    want = np.empty_like(img)
    want[:] = (9, 8, 7)
    want[2:, :9] = img[:10, 3:]
    wm = np.full((12, 12), -100, np.int64)
    wm[2:, :9] = mask[:10, 3:]
    assert np.array_equal(byts, want) and np.array_equal(ms, wm)


def test_half_pixel_shift_blends_neighbours_rounding_half_up():
    img = RNG.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    _, byts, _, _ = run1(img, (65536, 0, 32768, 0, 65536, 0) + CID, (6, 8))
    p = img.astype(np.int64)
    assert np.array_equal(byts, (p[:, :-1] + p[:, 1:] + 1) >> 1)
    _, byts, _, _ = run1(img, (65536, 0, 0, 0, 65536, 32768) + CID, (5, 9))
    assert np.array_equal(byts, (p[:-1] + p[1:] + 1) >> 1)


def test_colour_identities_and_both_clamps():
    img = RNG.integers(0, 256, (10, 14, 3), dtype=np.uint8)
    m = AO.mean_q8(AO.luma_sum(img), 140)
    A, k = mgunet.color_matrix_q12(1.0, 1.0, 0.0, 0.0)                         # s = 0: three equal channels
    _, byts, _, _ = run1(img, IDENT + A + (k,), (10, 14))
    assert np.array_equal(byts[..., 0], byts[..., 1]) and np.array_equal(byts[..., 1], byts[..., 2]) and len(np.unique(byts)) > 20
    for b in (1.0, 0.5):                                                          # c = 0: every pixel round(b m / 256)
        A, k = mgunet.color_matrix_q12(b, 0.0, 1.0, 0.0)
        _, byts, _, _ = run1(img, IDENT + A + (k,), (10, 14))
        assert A == (0,) * 9 and (byts == int(math.floor(b * m / 256.0 + 0.5))).all()
    A, k = mgunet.color_matrix_q12(0.0, 1.3, 0.7, 0.1)                         # b = 0: black
    _, byts, _, _ = run1(img, IDENT + A + (k,), (10, 14))
    assert not byts.any()
    A, k = mgunet.color_matrix_q12(1.2, 1.2, 1.0, 0.0)
    img[0, 0], img[0, 1] = (255, 255, 255), (0, 0, 0)
    _, byts, _, _ = run1(img, IDENT + A + (k,), (10, 14))
    q = img.astype(np.int64) @ np.asarray(A).reshape(3, 3).T + ((k * AO.mean_q8(AO.luma_sum(img), 140) + 128) >> 8) + 2048
    assert (q >> 12).max() > 255 and (q >> 12).min() < 0                         # both clamps are reached
    assert byts.max() == 255 and byts.min() == 0 and np.array_equal(byts, np.clip(q >> 12, 0, 255))
    # bgr: the same picture stored B, G, R gives the same result
    a = AO.augment(img[None], np.asarray([IDENT + A + (k,)]), (10, 14), AC.MEAN, AC.STD)[1]
    b = AO.augment(img[None, ..., ::-1], np.asarray([IDENT + A + (k,)]), (10, 14), AC.MEAN, AC.STD, bgr=True)[1]
    assert np.array_equal(a, b)


def test_mask_clip_and_fill():
    mask = np.asarray([[0, 1, 2, 5, 255]], np.uint8)
    img = np.zeros((1, 5, 3), np.uint8)
    tab = (65536, 0, -65536, 0, 65536, 0) + CID                                  # reads x - 1: the first output pixel lies outside
    assert run1(img, tab, (1, 5), mask, num_classes=2, mask_fill=-100)[3].tolist() == [[-100, 0, 1, 1, 1]]
    assert run1(img, tab, (1, 5), mask, num_classes=0, mask_fill=7)[3].tolist() == [[7, 0, 1, 2, 5]]


def test_oracle_against_float64_bilinear_on_every_case():
    """8-bit fractions move a coordinate by less than 1/256 px: less than one level per axis; plus 0.5 for the rounding"""
    worst, n = 0.0, 0
    for tag in AC.CASES:
        img, masks, table, c = AC.inputs(tag)
        smp = AC.reference(tag)[2]
        (Hs, Ws), out_hw = AC.SHAPES[c["shape"]]
        for b in range(len(c["names"])):
            rgb = img[b][..., ::-1] if c["bgr"] else img[b]
            inside = AO.interior((Hs, Ws), table[b].tolist(), out_hw)
            if inside.any():
                d = np.abs(smp[b].astype(np.float64) - AO.bilinear_f64(rgb, table[b].tolist(), out_hw))[inside]
                worst, n = max(worst, float(d.max())), n + int(inside.sum())
    print(f"oracle against float64 bilinear: max |diff| {worst:.4f} over {n} interior pixels")
    assert n > 100000 and worst < 2.5


# ---- color_matrix_q12, affine_fixed, draw ----------------------------------------------------------------------------------------------
def test_color_matrix_q12():
    assert mgunet.color_matrix_q12() == ((4096, 0, 0, 0, 4096, 0, 0, 0, 4096), 0)
    assert mgunet.color_matrix_q12(1, 1, 0, 0)[0] == (1232, 2400, 464) * 3
    for b, c, s, h in [(1.2, 0.8, 1.2, 0.02), (0.8, 1.2, 0.8, -0.02), (1.0, 1.0, 0.3, 0.5), (2.0, 2.0, 1.5, 0.25), (0.9, 1.1, 1.0, -0.4)]:
        A, k = mgunet.color_matrix_q12(b, c, s, h)
        want = int(math.floor(b * c * 4096 + 0.5))
        for r in range(3):
            assert abs(sum(A[3 * r:3 * r + 3]) - want) <= 2, (b, c, s, h)        # greys are preserved
        assert k == int(math.floor(b * (1 - c) * 4096 + 0.5))
    # the hue turn is a rotation about the grey axis: a third of a turn permutes the channels
    assert mgunet.color_matrix_q12(1, 1, 1, 1 / 3)[0] in ((0, 0, 4096, 4096, 0, 0, 0, 4096, 0), (0, 4096, 0, 0, 0, 4096, 4096, 0, 0))
    assert max(mgunet.color_matrix_q12(8.0, 1.0, 1.0, 0.0)[0]) == 1 << 15          # the limit itself passes
    for args in [(8.01, 1, 1, 0), (3, 3, 1, 0), (1, 9.5, 1, 0), (4, -1.1, 1, 0)]:
        with pytest.raises(ValueError, match="2\\^15"):
            mgunet.color_matrix_q12(*args)


def matrix_f64(flip, angle, zoom, aspect, tx, ty, src_hw, out_hw):
    """the float64 map of the docstring of affine_fixed, written independently: output pixel centre -> source pixel index"""
    (Hs, Ws), (H, W) = src_hw, out_hw
    cw, ch = (Ws / zoom, Hs / (zoom * aspect)) if aspect >= 1 else (Ws * aspect / zoom, Hs / zoom)
    th = math.radians(angle)
    cx, cy = Ws / 2 + tx * (Ws / 2) * (1 - 1 / zoom), Hs / 2 + ty * (Hs / 2) * (1 - 1 / zoom)

    def at(x, y):
        X, Y = ((x + 0.5) - W / 2) * cw / W * (-1 if flip else 1), ((y + 0.5) - H / 2) * ch / H
        return cx + math.cos(th) * X - math.sin(th) * Y - 0.5, cy + math.sin(th) * X + math.cos(th) * Y - 0.5
    return at


def test_affine_fixed_against_the_float64_matrix():
    assert mgunet.affine_fixed(0, 0.0, 1.0, 1.0, 0.0, 0.0, (48, 64), (48, 64)) == IDENT
    rng = np.random.default_rng(5)
    for _ in range(100):
        Hs, Ws, H, W = (int(v) for v in rng.integers(1, 700, 4))
        flip, angle = bool(rng.integers(0, 2)), float(rng.uniform(-180, 180))
        zoom, aspect = float(np.exp(rng.uniform(np.log(0.25), np.log(4)))), float(np.exp(rng.uniform(np.log(0.5), np.log(2))))
        tx, ty = (float(v) for v in rng.uniform(-1, 1, 2))
        a = mgunet.affine_fixed(flip, angle, zoom, aspect, tx, ty, (Hs, Ws), (H, W))
        at = matrix_f64(flip, angle, zoom, aspect, tx, ty, (Hs, Ws), (H, W))
        for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            u, v = at(x, y)
            sx, sy = a[2] + y * a[1] + x * a[0], a[5] + y * a[4] + x * a[3]
            assert abs(sx / 65536 - u) <= (W + H) / 65536 and abs(sy / 65536 - v) <= (W + H) / 65536, (Hs, Ws, H, W, angle, zoom)
    with pytest.raises(ValueError):
        mgunet.affine_fixed(0, 0, 1, 1, 0, 0, (8193, 4), (4, 4))
    with pytest.raises(ValueError, match="int32"):
        mgunet.affine_fixed(0, 0, 1e-5, 1, 0, 0, (8192, 8192), (2, 2))


def test_zoomed_in_unrotated_crops_stay_inside_the_source():
    """zoom >= 1, angle 0, any aspect and crop position, a result no larger than a third of the crop: every tap of every pixel lies inside
    the source (the outermost sample centres sit at least a pixel inside the crop, which lies inside the source)"""
    g = torch.Generator().manual_seed(3)
    src, out = (96, 128), (16, 20)
    for _ in range(200):
        r = torch.rand(6, dtype=torch.float64, generator=g).tolist()
        zoom, aspect = math.exp(r[2] * math.log(2.0)), math.exp(math.log(3 / 4) + r[3] * (math.log(4 / 3) - math.log(3 / 4)))
        a = mgunet.affine_fixed(r[0] < 0.5, 0.0, zoom, aspect, 2 * r[4] - 1, 2 * r[5] - 1, src, out)
        assert AO.interior(src, a + CID, out).all(), (zoom, aspect, r)
    assert not AO.interior(src, mgunet.affine_fixed(0, 0.0, 0.9, 1.0, 0, 0, src, out) + CID, out).all()


def test_draw_order_and_generator_advance():
    aug = mgunet.RandomAffineColor((24, 40), degrees=20, p_flip=0.3, hue=0.05)
    src = (50, 70)
    t = aug.draw(5, src, generator=torch.Generator().manual_seed(9))
    assert t.dtype == torch.int32 and tuple(t.shape) == (5, 16)
    g = torch.Generator().manual_seed(9)
    lu = lambda lo, hi, u: math.exp(math.log(lo) + u * (math.log(hi) - math.log(lo)))
    for i in range(5):
        r = torch.rand(10, dtype=torch.float64, generator=g).tolist()
        fix = mgunet.affine_fixed(r[0] < 0.3, (2 * r[1] - 1) * 20, lu(0.5, 2.0, r[2]), lu(3 / 4, 4 / 3, r[3]), 2 * r[4] - 1, 2 * r[5] - 1, src, (24, 40))
        A, k = mgunet.color_matrix_q12(1 + (2 * r[6] - 1) * 0.2, 1 + (2 * r[7] - 1) * 0.2, 1 + (2 * r[8] - 1) * 0.2, (2 * r[9] - 1) * 0.05)
        assert tuple(t[i].tolist()) == fix + A + (k,), i
    g2 = torch.Generator().manual_seed(9)
    aug.draw(5, src, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())                             # exactly B draws of ten
    # disabled terms still consume their entries: the enabled ones see the same draws
    off = mgunet.RandomAffineColor((24, 40), degrees=20, p_flip=0.0, brightness=0, contrast=0, saturation=0, hue=0)
    t0 = off.draw(5, src, generator=torch.Generator().manual_seed(9))
    assert torch.equal(t0[:, 6:], torch.tensor(CID, dtype=torch.int32).repeat(5, 1))
    g3 = torch.Generator().manual_seed(9)
    for i in range(5):
        r = torch.rand(10, dtype=torch.float64, generator=g3).tolist()
        assert tuple(t0[i, :6].tolist()) == mgunet.affine_fixed(False, (2 * r[1] - 1) * 20, lu(0.5, 2.0, r[2]), lu(3 / 4, 4 / 3, r[3]), 2 * r[4] - 1,
                                                                2 * r[5] - 1, src, (24, 40))
    # the global generator serves when none is given
    torch.manual_seed(4)
    a = aug.draw(2, src)
    torch.manual_seed(4)
    assert torch.equal(a, aug.draw(2, src))


# ---- the cases tell wrong readings apart ---------------------------------------------------------------------------------------------
def test_case_table_covers_what_the_gpu_tier_runs():
    shapes = {c["shape"] for c in AC.CASES.values()}
    assert shapes == set(AC.SHAPES) and {len(c["names"]) for c in AC.CASES.values()} == {1, 3}
    for shape in AC.SHAPES:
        if shape != "512":
            assert {n for c in AC.CASES.values() if c["shape"] == shape for n in c["names"]} == set(AC.NAMES), shape
    assert {c["num_classes"] for c in AC.CASES.values()} == {0, 2} and any(c["bgr"] for c in AC.CASES.values())
    assert max(abs(v) for v in AC.row("limit_pos", (4, 4), (4, 4))[6:]) == 1 << 15
    # zoom 0.5 leaves fill on all four sides; both clamps occur in the limit tables
    ms = AC.reference("64x64/zoom_half")[3][0]
    assert (ms[0] == -100).all() and (ms[-1] == -100).all() and (ms[:, 0] == -100).all() and (ms[:, -1] == -100).all() and (ms[32] != -100).any()
    assert AC.reference("64x64/limit_pos")[1].max() == 255 and AC.reference("64x64/limit_mix")[1].min() == 0
    assert [hw[0] * hw[1] for hw in AC.luma_shapes(4096)] == [1, 255, 256, 257, 4095, 4096, 4097, 8195]


@pytest.mark.parametrize("variant", AO.VARIANTS)
def test_cases_tell_wrong_readings_of_the_definition_apart(variant):
    told = []
    for tag in AC.CASES:
        right, wrong = AC.reference(tag), AC.reference(tag, variant)
        if not (np.array_equal(right[1], wrong[1]) and np.array_equal(right[3], wrong[3])):
            told.append(tag)
    print(f"{variant}: told apart by {len(told)} of {len(AC.CASES)} cases, e.g. {told[:4]}")
    assert told, variant
    if variant == "int32_wrap":      # at a case with zoom != 1 on a source at least 256 wide
        assert "512/three" in told and AC.SHAPES["512"][0][1] >= 256
