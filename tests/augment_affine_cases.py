"""Cases of the affine + colour augmentation shared by the host tier (tests/test_augment_affine_host.py: oracle properties, float64
bilinear, wrong variants) and the GPU tier (tests/test_gpu_augment_affine.py: bitwise equality).  A case is a batch of B source images
with one named transform per image; its integer table comes from mgunet.affine_fixed / color_matrix_q12 (checked against float64 in
the host tier) or is written out (the tables at the limits).  Inputs are seeded by the tag; references are computed once."""
import functools
import math
import zlib
from collections import OrderedDict

import numpy as np

import mgunet
import augment_affine_oracle as AO

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FILL = (124, 116, 104)          # a visible fill, so that fill against edge-clamp and its colour jitter show
MASK_FILL = -100

SHAPES = OrderedDict([          # (Hs, Ws) -> (H, W)
    ("1x1", ((1, 1), (1, 1))), ("5x7", ((5, 7), (3, 9))), ("33x35", ((33, 35), (32, 32))),
    ("40x24", ((40, 24), (33, 35))),      # scalar path, ragged tiles
    ("64x64", ((64, 64), (64, 64))),      # vector path
    ("96x80", ((96, 80), (64, 128))), ("512", ((512, 512), (256, 256)))])

ID = dict(flip=0, angle=0.0, zoom=1.0, aspect=1.0, tx=0.0, ty=0.0, b=1.0, c=1.0, s=1.0, h=0.0)
Q = 1 << 15
IDENT_ROW = (65536, 0, 0, 0, 65536, 0, 4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0)      # reads the source pixel of the same index, colours unchanged
TRANSFORMS = OrderedDict([
    ("identity", {}), ("flip", dict(flip=1)), ("rot_p15", dict(angle=15.0)), ("rot_m15", dict(angle=-15.0)), ("rot90", dict(angle=90.0)),
    ("zoom_half", dict(zoom=0.5)), ("zoom_two", dict(zoom=2.0)), ("aspect_wide", dict(aspect=4 / 3)), ("aspect_tall", dict(aspect=3 / 4)),
    ("crop_nw", dict(zoom=2.0, tx=-1.0, ty=-1.0)), ("crop_se", dict(zoom=2.0, tx=1.0, ty=1.0)), ("crop_ne", dict(zoom=2.0, tx=1.0, ty=-1.0)),
    ("crop_sw", dict(zoom=2.0, tx=-1.0, ty=1.0)),
    ("bright_lo", dict(b=0.8)), ("bright_hi", dict(b=1.2)), ("contrast_lo", dict(c=0.8)), ("contrast_hi", dict(c=1.2)),
    ("sat_lo", dict(s=0.8)), ("sat_hi", dict(s=1.2)), ("hue_lo", dict(h=-0.02)), ("hue_hi", dict(h=0.02)),
    # tables at the 2^15 limit: every entry +2^15 (white wherever a byte is set), and a signed mix with k = -2^15
    ("limit_pos", dict(table=(65536, 0, 0, 0, 65536, 0) + (Q,) * 9 + (Q,))),
    ("limit_mix", dict(table=(65536, 0, 0, 0, 65536, 0) + (Q, -Q, 0, -Q, Q, -Q, 0, Q, -Q) + (-Q,))),
    # a0 = 2^30: from x = 2 on the coordinate sum passes 2^31; in 32 bits x = 4 would come back to column 0
    ("far", dict(table=(1 << 30, 0, 0, 0, 65536, 0, 4096, 0, 0, 0, 4096, 0, 0, 0, 4096, 0))),
    ("combined", dict(flip=1, angle=11.0, zoom=0.7, aspect=1.2, tx=0.6, ty=-0.8, b=1.15, c=0.85, s=1.2, h=0.015)),
    ("combined2", dict(angle=-13.0, zoom=1.6, aspect=0.8, tx=-1.0, ty=0.5, b=0.9, c=1.2, s=0.8, h=-0.02)),
    ("zoom_half_dark", dict(zoom=0.5, angle=15.0, b=0.8, c=1.2)),
])
NAMES = list(TRANSFORMS)


def row(name, src_hw, out_hw) -> tuple:
    """the 16 table entries of a named transform at these sizes"""
    t = TRANSFORMS[name]
    if "table" in t:
        return tuple(t["table"])
    p = dict(ID, **t)
    A, k = mgunet.color_matrix_q12(p["b"], p["c"], p["s"], p["h"])
    return mgunet.affine_fixed(p["flip"], p["angle"], p["zoom"], p["aspect"], p["tx"], p["ty"], src_hw, out_hw) + A + (k,)


def cases() -> OrderedDict:
    """tag -> dict(shape, names (one transform per image), num_classes, bgr)"""
    cs = OrderedDict()
    for shape in SHAPES:
        if shape == "512":
            continue
        for g in range(0, len(NAMES), 3):         # B = 3, another transform per image: every transform at every shape
            cs[f"{shape}/g{g // 3}"] = dict(shape=shape, names=NAMES[g:g + 3], num_classes=(0, 2)[(g // 3) % 2], bgr=(g // 3) % 4 == 3)
        cs[f"{shape}/one"] = dict(shape=shape, names=["combined"], num_classes=2, bgr=False)
    for shape in ("40x24", "64x64"):              # B = 1: each transform alone, on the scalar and on the vector path
        for n in NAMES:
            cs[f"{shape}/{n}"] = dict(shape=shape, names=[n], num_classes=(2, 0)[NAMES.index(n) % 2], bgr=False)
    cs["512/three"] = dict(shape="512", names=["combined", "far", "zoom_half_dark"], num_classes=2, bgr=False)
    return cs


CASES = cases()


def inputs(tag):
    """-> (images (B, Hs, Ws, 3) uint8, masks (B, Hs, Ws) uint8 with bytes above any class count, table (B, 16) int64, case)"""
    c = CASES[tag]
    (Hs, Ws), out_hw = SHAPES[c["shape"]]
    B = len(c["names"])
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    img = rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)
    if Hs >= 32:                                  # a smooth half, so that interpolation is not only noise
        yy, xx = np.mgrid[0:Hs, 0:Ws]
        img[:, :, : Ws // 2, 1] = ((np.sin(yy / 7.0) * np.cos(xx / 5.0) * 0.5 + 0.5) * 255).astype(np.uint8)[:, : Ws // 2]
    masks = rng.integers(0, 6, (B, Hs, Ws), dtype=np.uint8)
    masks[rng.random((B, Hs, Ws)) < 0.05] = 255
    table = np.asarray([row(n, (Hs, Ws), out_hw) for n in c["names"]], np.int64)
    return img, masks, table, c


@functools.lru_cache(maxsize=None)
def reference(tag, variant=None):
    """(out float32 (B, 3, H, W), bytes, sampled bytes, masks int64) of the oracle (or of a wrong variant of it); shared, read-only"""
    img, masks, table, c = inputs(tag)
    r = AO.augment(img, table, SHAPES[c["shape"]][1], MEAN, STD, masks=masks, fill=FILL, mask_fill=MASK_FILL, num_classes=c["num_classes"],
                   bgr=c["bgr"], variant=variant)
    for a in r:
        a.setflags(write=False)
    return r


def luma_shapes(T):
    """(Hs, Ws) with Hs Ws = n for the pixel counts around the luma kernel's tile T, both sides <= 8192"""
    out = []
    for n in (1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3):
        h = max(d for d in range(1, int(math.isqrt(n)) + 1) if n % d == 0)
        assert n // h <= 8192, n
        out.append((h, n // h))
    return out
