"""Cases of the elastic deformation shared by the host tier (tests/test_augment_elastic_host.py: oracle properties, wrong variants,
coverage) and the GPU tier (tests/test_gpu_augment_elastic.py: bitwise equality).  A case is a batch of B source images with one table
row and one control field per image.  The shapes are the smallest at which the kernel can still go wrong; inputs are seeded by the tag
and references are computed once."""
import functools
import zlib
from collections import OrderedDict

import numpy as np

import mgunet
import augment_affine_cases as AC
import augment_elastic_oracle as EO

MEAN, STD, FILL, MASK_FILL = AC.MEAN, AC.STD, AC.FILL, AC.MASK_FILL
LABEL_FILL = -7
SIGMA = 3.0
LABEL_IDS = np.asarray([0, 1, 2, 3, (1 << 24) + 5, (1 << 30) + 7, -3, -(1 << 28)], np.int32)      # beyond float32's integers, and negative

SHAPES = OrderedDict([          # (Hs, Ws) -> (H, W), (gh, gw)
    ("5x7", ((5, 7), (5, 7), (4, 4))),            # one cell, ragged tile, scalar stores
    ("40x24", ((40, 24), (33, 65), (6, 5))),      # crosses the 32-pixel tile edge on both axes; su, sv no powers of two
    ("24x40", ((24, 40), (64, 64), (7, 7))),      # vector stores
    ("16x16", ((16, 16), (32, 32), (32, 32))),    # cells of at most one pixel: every lattice index is used
    ("9x11", ((9, 11), (7, 7), (4, 6))),          # W = 7: su = floor(3 * 65536 / 7), where floor and round part
])
# the seeded fields go through a rotated, zoomed, flipped row with a colour jitter (k != 0: the luma pass runs)
WARP = dict(flip=1, angle=11.0, zoom=1.3, aspect=1.1, tx=0.3, ty=-0.2, b=1.1, c=0.9, s=1.1, h=0.01)
CONST = ((3 << 16) + 12345, -((1 << 16) + 54321))
FIELDS = ("zero", "const", "spike", "seeded")
ROWS = dict(zero="combined", const="rot_m15", spike="rot_p15", seeded="warp")
BATCH = (("const", "combined2"), ("spike", "identity"), ("seeded", "warp"))      # B = 3: another field and row per image


def row(name, src_hw, out_hw) -> tuple:
    if name != "warp":
        return AC.row(name, src_hw, out_hw)
    A, k = mgunet.color_matrix_q12(WARP["b"], WARP["c"], WARP["s"], WARP["h"])
    return mgunet.affine_fixed(WARP["flip"], WARP["angle"], WARP["zoom"], WARP["aspect"], WARP["tx"], WARP["ty"], src_hw, out_hw) + A + (k,)


def control_field(kind, nodes, table_row, rng) -> np.ndarray:
    """int64 (2, gh, gw)"""
    gh, gw = nodes
    c = np.zeros((2, gh, gw), np.int64)
    if kind == "const":
        c[0], c[1] = CONST
    elif kind == "spike":
        # one node at +2^26 beside one at -2^26 (x: neighbours along the row, y: along the column), once per 8 x 8 nodes, so that the
        # fine grid leaves the source over a tenth of its pixels as the coarse ones do
        for j in range(1, gh - 1, 8):
            for i in range(1, gw - 1, 8):
                c[0, j, i], c[0, j, i + 1] = EO.CTRL_LIMIT, -EO.CTRL_LIMIT
                c[1, j, i], c[1, j + 1, i] = -EO.CTRL_LIMIT, EO.CTRL_LIMIT
    elif kind == "seeded":
        c[:] = np.asarray(EO.control(rng.standard_normal((2, gh, gw)), SIGMA, table_row), np.int64)
    return c


def cases() -> OrderedDict:
    """tag -> dict(shape, fields, rows, num_classes, bgr)"""
    cs = OrderedDict()
    for n, shape in enumerate(SHAPES):
        for f in FIELDS:
            cs[f"{shape}/{f}"] = dict(shape=shape, fields=[f], rows=[ROWS[f]], num_classes=(0, 2)[(n + FIELDS.index(f)) % 2], bgr=False)
        cs[f"{shape}/batch"] = dict(shape=shape, fields=[f for f, _ in BATCH], rows=[r for _, r in BATCH], num_classes=(2, 0)[n % 2], bgr=n == 1)
    return cs


CASES = cases()
SEEDED = [t for t in CASES if t.endswith("/seeded")]
SPIKE = [t for t in CASES if t.endswith("/spike")]


def inputs(tag):
    """-> (images (B, Hs, Ws, 3) uint8, masks (B, Hs, Ws) uint8, labels (B, Hs, Ws) int32, table (B, 16) int64, ctrl (B, 2, gh, gw) int64, case)"""
    c = CASES[tag]
    (Hs, Ws), out_hw, nodes = SHAPES[c["shape"]]
    B = len(c["fields"])
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    img = rng.integers(0, 256, (B, Hs, Ws, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:Hs, 0:Ws]                     # a smooth half, so that interpolation is not only noise
    img[:, :, : Ws // 2, 1] = ((np.sin(yy / 7.0) * np.cos(xx / 5.0) * 0.5 + 0.5) * 255).astype(np.uint8)[:, : Ws // 2]
    masks = rng.integers(0, 6, (B, Hs, Ws), dtype=np.uint8)
    masks[rng.random((B, Hs, Ws)) < 0.05] = 255
    labels = LABEL_IDS[rng.integers(0, len(LABEL_IDS), (B, Hs, Ws))]
    table = np.asarray([row(n, (Hs, Ws), out_hw) for n in c["rows"]], np.int64)
    ctrl = np.stack([control_field(f, nodes, table[b].tolist(), rng) for b, f in enumerate(c["fields"])])
    return img, masks, labels, table, ctrl, c


@functools.lru_cache(maxsize=None)
def reference(tag, variant=None):
    """(out float32 (B, 3, H, W), bytes, masks int64, labels int32, field int64 (B, 2, H, W)) of the oracle (or of a wrong variant of it);
    shared, read-only"""
    img, masks, labels, table, ctrl, c = inputs(tag)
    out_hw = SHAPES[c["shape"]][1]
    r = EO.augment(img, table, ctrl, out_hw, MEAN, STD, masks=masks, labels=labels, fill=FILL, mask_fill=MASK_FILL, label_fill=LABEL_FILL,
                   num_classes=c["num_classes"], bgr=c["bgr"], variant=variant)
    r = r + (np.stack([np.stack(EO.field(ctrl[b], out_hw, variant)) for b in range(len(ctrl))]),)
    for a in r:
        a.setflags(write=False)
    return r
