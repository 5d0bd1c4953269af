"""Designed cases of csrc/objects.hip -- the union-find labelling and the greedy box matching -- shared by the host tier
(tests/test_objects_cases_host.py) and the GPU tier (tests/test_gpu_objects_scenes.py, tests/test_gpu_match_objects.py).  Everything
is built from index arithmetic and seeded numpy generators; nothing is read from disk.

Labelling scenes are int64 class maps, each there for one shape the tile pass or the border pass can get wrong; the reference is
objects_oracle.label / stats.  Matching cases are hand-built object tables (class and box per object) in which one named wrong
decision changes the number of matched GT objects; the reference is the plain greedy loop match_reference below.  tiled_label and
match_variant restate the kernels with one decision switched, so that the host tier can show every case catches what it is for."""
import functools
import math

import numpy as np

import objects_oracle as OO

TILE = 32      # csrc/objects.hip: labelling tile, TILE x TILE pixels
CHUNK = 1024   # csrc/objects.hip: pixels of one image per root-numbering workgroup
LANES = 64     # match_kernel: GT object j belongs to lane j % 64
SCAN_THREADS = 1024   # objects_common.h: threads of chunk_sum_scan, each with ceil(n / 1024) chunk counts

SIZES = [(96, 96), (70, 45), (130, 161)]   # 3 x 3 whole tiles; two ragged sizes (3 x 2 and 5 x 6 tiles)


# ---- labelling scenes -------------------------------------------------------------------------------------------------------------
def _grid(H, W):
    return np.arange(H)[:, None], np.arange(W)[None, :]


def row_serpentine(H, W):
    """every second row full, joined alternately at the right and the left end"""
    y, x = _grid(H, W)
    return ((y % 2 == 0) | ((y % 4 == 1) & (x == W - 1)) | ((y % 4 == 3) & (x == 0))).astype(np.int64)


def col_serpentine(H, W):
    """vertical bars joined alternately at the bottom and the top: a bar meets its left neighbour only in its last or first pixel"""
    y, x = _grid(H, W)
    return ((x % 2 == 0) | ((x % 4 == 1) & (y == H - 1)) | ((x % 4 == 3) & (y == 0))).astype(np.int64)


def comb(H, W):
    """teeth two pixels apart, joined only by the last row"""
    y, x = _grid(H, W)
    return ((x % 2 == 0) | (y == H - 1)).astype(np.int64)


def spiral(H, W):
    """a square spiral one pixel wide with one-pixel gaps, walked inwards from (0, 0)"""
    p = np.zeros((H + 2, W + 2), np.int64)   # the map inside a background frame: pixel (y, x) is p[y + 1, x + 1]
    y = x = 1
    dy, dx = 0, 1
    p[1, 1] = 1
    while True:
        for _ in range(2):                   # a step is taken when the new pixel touches the path in the current pixel alone
            ny, nx = y + dy, x + dx
            if 1 <= ny <= H and 1 <= nx <= W and not p[ny, nx] and p[ny - 1, nx] + p[ny + 1, nx] + p[ny, nx - 1] + p[ny, nx + 1] == 1:
                break
            dy, dx = dx, -dy                 # turn right
        else:
            return p[1:-1, 1:-1].copy()
        y, x = ny, nx
        p[y, x] = 1


def rings(H, W):
    """concentric one-pixel square rings with one-pixel gaps"""
    y, x = _grid(H, W)
    return (np.minimum(np.minimum(y, H - 1 - y), np.minimum(x, W - 1 - x)) % 2 == 0).astype(np.int64)


def with_complement(m):
    """the path as class 1, everything else as class 2: two interleaved sets of components that never join across"""
    return np.where(m > 0, 1, 2).astype(np.int64)


def anti_sum(H):
    """x + y of the anti-diagonal that passes through the tile corners (32 k, 32 (K - k)), K = H // TILE"""
    return TILE * (H // TILE) - 1


def diagonal(H, W, kind, shift=0):
    """'main': x = y + shift; 'anti': x + y = anti_sum(H) + shift; 'x': both.  shift 0 passes exactly through tile corners (the
    join exists through the diagonal tile alone), shift 1 crosses tile edges one pixel away from them."""
    y, x = _grid(H, W)
    main, anti = x == y + shift, x + y == anti_sum(H) + shift
    return {"main": main, "anti": anti, "x": main | anti}[kind].astype(np.int64)


def tile_corners(H, W):
    """the interior tile corners (cy, cx): the 2 x 2 block around one is rows cy - 1, cy and columns cx - 1, cx"""
    return [(cy, cx) for cy in range(TILE, H, TILE) for cx in range(TILE, W, TILE)]


def corner_contacts(H, W, kind):
    """'nwse': at every interior tile corner only the NW and SE pixels of the 2 x 2 block; 'nesw': only the NE and SW pixels"""
    m = np.zeros((H, W), np.int64)
    for cy, cx in tile_corners(H, W):
        if kind == "nwse":
            m[cy - 1, cx - 1] = m[cy, cx] = 1
        else:
            m[cy - 1, cx] = m[cy, cx - 1] = 1
    return m


EDGE_POSITIONS = (0, TILE // 2, TILE - 1)   # first, middle and last position of a tile edge


def edge_contacts(H, W, kind):
    """three pairs of rectangles in neighbouring tiles, each pair touching through exactly one 4-neighbour pixel pair, placed at the
    first, middle and last position of the shared tile edge.  'h': horizontally adjacent tiles of tile row 1 (an 8 x 1 bar ending
    at column 31 against a block 4 high and 7 wide from column 32); 'v': vertically adjacent tiles (a 1 x 8 bar ending at row 63
    against a 4 x 4 block from row 64) of tile column 1 where the map has one whole, else of tile column 0."""
    m = np.zeros((H, W), np.int64)
    for p in EDGE_POSITIONS:
        lo = min(p, TILE - 4)   # the block's 4 positions along the edge contain p
        if kind == "h":
            r = TILE + p
            m[r, TILE - 8:TILE] = 1
            m[TILE + lo:TILE + lo + 4, TILE:TILE + 7] = 1
        else:
            c0 = TILE if W >= 2 * TILE else 0
            m[2 * TILE - 8:2 * TILE, c0 + p] = 1
            m[2 * TILE:2 * TILE + 4, c0 + lo:c0 + lo + 4] = 1
    return m


PATHS = {"row_serpentine": row_serpentine, "col_serpentine": col_serpentine, "comb": comb, "spiral": spiral}

SCENES = {}
for _n, _f in PATHS.items():
    SCENES[_n] = _f
    SCENES[_n + "_compl"] = (lambda f: lambda H, W: with_complement(f(H, W)))(_f)
SCENES["rings"] = rings
SCENES["rings_compl"] = lambda H, W: with_complement(rings(H, W))
for _k in ("main", "anti", "x"):
    for _s in (0, 1):
        SCENES[f"diag_{_k}{'_shift' if _s else ''}"] = (lambda k, s: lambda H, W: diagonal(H, W, k, s))(_k, _s)
for _k in ("nwse", "nesw"):
    SCENES["corner_" + _k] = (lambda k: lambda H, W: corner_contacts(H, W, k))(_k)
for _k in ("h", "v"):
    SCENES["edge_" + _k] = (lambda k: lambda H, W: edge_contacts(H, W, k))(_k)
SCENE_NAMES = list(SCENES)
REGION_SCENES = [n for n in SCENE_NAMES if not n.startswith(("rings", "edge"))]   # path, diagonal and corner scenes, as raw label maps


@functools.lru_cache(maxsize=None)
def scene(name, size):
    m = SCENES[name](*size)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def scene_batch(size):
    """every scene of one size as one (B, H, W) batch, in SCENE_NAMES order"""
    m = np.stack([scene(n, size) for n in SCENE_NAMES])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def expected(name, size, connectivity, min_area=0):
    """(labels, (class, area, bbox, sums)) of one scene from the oracle, computed once"""
    m = scene(name, size)
    lab = OO.label(m, connectivity, min_area=min_area)
    lab.setflags(write=False)
    return lab, OO.stats(lab, m)


def table_of(labels, maps):
    """the oracle's whole table of a labelled batch: (counts, offsets, class, area, bbox, sums), rows in batch-wide object order"""
    per = [OO.stats(lab, m) for lab, m in zip(labels, maps)]
    counts = np.array([lab.max(initial=0) for lab in labels], np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cls, area, bbox, sums = (np.concatenate([p[k] for p in per]) for k in range(4))
    return counts, offsets, cls, area, bbox, sums


# ---- min_area at exact areas ------------------------------------------------------------------------------------------------------
AREAS = range(1, 71)
AREA_MAP_SIZE = (105, 161)
MIN_AREAS = (1, 63, 64, 65, 71)


@functools.lru_cache(maxsize=None)
def area_map():
    """separated rectangles of areas 1..70 (2 rows x a/2 for an even a >= 4, else 1 x a), classes alternating 1 and 2: area a sits at
    row 3 ((a - 1) % 35) and column 0 (a <= 35) or 80"""
    m = np.zeros(AREA_MAP_SIZE, np.int64)
    for a in AREAS:
        h, w = (2, a // 2) if a % 2 == 0 and a >= 4 else (1, a)
        y0, x0 = 3 * ((a - 1) % 35), 0 if a <= 35 else 80
        assert not m[y0:y0 + h, x0:x0 + w].any()
        m[y0:y0 + h, x0:x0 + w] = 1 + a % 2
    m.setflags(write=False)
    return m


# ---- large batches ----------------------------------------------------------------------------------------------------------------
LARGE_BATCHES = [(1025, 3, 5), (2049, 3, 5), (700, 30, 50)]   # chunk counts n = 1025, 2049, 1400: scan segments of 2, 3 and 2 chunks


def scan_segment(B, H, W):
    """(n, seg): chunk counts of the batch and the number each thread of chunk_sum_scan sums"""
    n = B * -(-H * W // CHUNK)
    return n, -(-n // SCAN_THREADS)


@functools.lru_cache(maxsize=None)
def random_batch(B, H, W):
    m = (np.random.default_rng(B + 31 * H + W).random((B, H, W)) < 0.5).astype(np.int64)
    m.setflags(write=False)
    return m


def stacked_table(maps, connectivity):
    """(labels (B, H, W), counts, offsets, class, area, bbox, sums) of a batch of many small maps from ONE oracle call: the images
    stacked vertically with a background row between them.  The oracle numbers objects in raster order of their first pixel, so
    image b's objects are a run of the stacked numbering and keep their order; y moves back by b (H + 1)."""
    B, H, W = maps.shape
    tall = np.zeros((B, H + 1, W), np.int64)
    tall[:, :H] = maps
    tall = tall.reshape(B * (H + 1), W)
    lab = OO.label(tall, connectivity)
    cls, area, bbox, sums = OO.stats(lab, tall)
    lab = lab.reshape(B, H + 1, W)[:, :H]
    offsets = np.concatenate([[0], np.maximum.accumulate(lab.reshape(B, -1).max(1))]).astype(np.int64)
    counts = np.diff(offsets)
    image = np.repeat(np.arange(B), counts)
    bbox, sums = bbox.copy(), sums.copy()
    bbox[:, 1] -= image * (H + 1)
    bbox[:, 3] -= image * (H + 1)
    sums[:, 1] -= area * image * (H + 1)
    labels = np.where(lab > 0, lab - offsets[:-1, None, None], 0).astype(np.int32)
    return labels, counts, offsets, cls, area, bbox, sums


def single_pixel_batch(B=65535):
    """(maps (B, 1, 1), labels, counts, offsets) of B one-pixel images, every other one foreground -- written down directly"""
    fg = (np.arange(B) % 2 == 0).astype(np.int64)
    return fg.reshape(B, 1, 1), fg.reshape(B, 1, 1).astype(np.int32), fg, np.concatenate([[0], np.cumsum(fg)]).astype(np.int64)


# ---- the tiled labelling restated, with one decision switched ---------------------------------------------------------------------
def _components(fg, u, v):
    """int64 (n,): the smallest index of every foreground element's component under the joins (u, v); -1 on background"""
    n = fg.size
    par = np.where(fg, np.arange(n), -1)
    while True:
        while True:
            nxt = np.where(par >= 0, par[np.maximum(par, 0)], -1)
            if np.array_equal(nxt, par):
                break
            par = nxt
        ru, rv = par[u], par[v]
        diff = ru != rv
        if not diff.any():
            return par
        np.minimum.at(par, np.maximum(ru[diff], rv[diff]), np.minimum(ru[diff], rv[diff]))


LABEL_VARIANTS = ("kernel", "border4", "no_up_right", "no_last_column")


def tiled_label(m, connectivity, variant="kernel"):
    """The labels the tile pass and the border pass of csrc/objects.hip produce on one (H, W) map, from the joins they make: the
    tile pass joins every pixel to its earlier neighbours inside its tile; the border pass joins the pixels of a tile's first row,
    first column and last column to their earlier neighbours in another tile.  Variants: 'kernel' as written; 'border4' a border
    pass that joins only 4-neighbours; 'no_up_right' one without the (y - 1, x + 1) neighbour; 'no_last_column' one that visits
    only the first row and the first column."""
    m = np.asarray(m)
    H, W = m.shape
    fg = m != 0
    idx = np.arange(H * W).reshape(H, W)
    y, x = _grid(H, W)
    us, vs = [], []
    for dy, dx in OO.OFFSETS[connectivity]:
        yy, xx = y + dy, x + dx
        ok = (yy >= 0) & (xx >= 0) & (xx < W)
        same_tile = (yy // TILE == y // TILE) & (xx // TILE == x // TILE)
        visited = (y % TILE == 0) | (x % TILE == 0)
        if variant != "no_last_column":
            visited = visited | (x % TILE == TILE - 1)
        border = visited & ~same_tile
        if (variant == "border4" and dy and dx) or (variant == "no_up_right" and (dy, dx) == (-1, 1)):
            border = border & False
        take = ok & (same_tile | border)
        a, b = np.nonzero(take)
        na, nb = a + dy, b + dx
        join = fg[a, b] & fg[na, nb] & (m[a, b] == m[na, nb])
        us.append(idx[a[join], b[join]])
        vs.append(idx[na[join], nb[join]])
    par = _components(fg.reshape(-1), np.concatenate(us), np.concatenate(vs))
    roots = par == np.arange(H * W)
    num = np.cumsum(roots)
    return np.where(par >= 0, num[np.maximum(par, 0)], 0).reshape(H, W).astype(np.int32)


def numbered_without_image_offset(labels):
    """a batch's labels as a numbering kernel would write them that takes the chunk's batch-wide object index and does not subtract
    the image's offset"""
    counts = np.array([lab.max(initial=0) for lab in labels], np.int64)
    before = np.concatenate([[0], np.cumsum(counts)])[:-1]
    return np.where(labels > 0, labels + before[:, None, None], 0).astype(np.int32)


# the scenes each wrong labelling must show on: (scene, size, connectivity)
LABEL_MUTANT_SCENES = {
    "border4": [("diag_main", (96, 96), 2), ("diag_anti", (96, 96), 2), ("diag_main_shift", (96, 96), 2), ("diag_anti_shift", (96, 96), 2),
                ("corner_nwse", (96, 96), 2), ("corner_nesw", (96, 96), 2), ("diag_x", (130, 161), 2)],
    "no_up_right": [("diag_anti", (96, 96), 2), ("diag_anti_shift", (96, 96), 2), ("corner_nesw", (96, 96), 2), ("corner_nesw", (70, 45), 2)],
    "no_last_column": [("diag_anti_shift", (96, 96), 2), ("diag_anti_shift", (70, 45), 2), ("diag_anti_shift", (130, 161), 2)],
}


# ---- matching: the reference and its variants -------------------------------------------------------------------------------------
def iou(a, b):
    """IoU of two [xmin, ymin, xmax, ymax) integer boxes as inter / union in Python floats (one correctly rounded quotient of two
    integers, as the kernel's double division of the same integers); 0.0 without an intersection"""
    iw, ih = max(0, min(a[2], b[2]) - max(a[0], b[0])), max(0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = iw * ih
    if inter == 0:
        return 0.0
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


MATCH_VARIANTS = ("kernel", "tie_last", "tie_lowest_lane", "first_candidate", "no_used", "strict_threshold", "no_class", "mark_below")


def match_variant(gt, pred, thresh, variant="kernel"):
    """Matched GT objects of one image.  gt, pred: lists of (class, box) of Python ints.  'kernel' is the greedy rule itself:
    predictions in order, each takes the unused GT object of its class with the largest IoU (the first of equals), if that IoU is
    positive and >= thresh.  The other variants switch one decision: 'tie_last' the last of equals; 'tie_lowest_lane' among equals
    the one in the lowest lane j % 64 (the first within a lane); 'first_candidate' the first overlapping candidate whatever its
    IoU; 'no_used' GT objects are never marked; 'strict_threshold' IoU > thresh; 'no_class' any class; 'mark_below' the best
    candidate is marked used even when it misses the threshold."""
    used = [False] * len(gt)
    matched = 0
    for pc, pb in pred:
        best, bj, blane = 0.0, -1, LANES
        for j, (gc, gb) in enumerate(gt):
            if used[j] or (gc != pc and variant != "no_class"):
                continue
            v = iou(pb, gb)
            if v == 0.0:
                continue
            if variant == "first_candidate":
                if bj < 0:
                    best, bj = v, j
            elif variant == "tie_lowest_lane":
                if v > best or (v == best and j % LANES < blane):
                    best, bj, blane = v, j, j % LANES
            elif v > best or (variant == "tie_last" and v == best):
                best, bj = v, j
        ok = bj >= 0 and (best > thresh if variant == "strict_threshold" else best >= thresh)
        if ok:
            matched += 1
        if bj >= 0 and variant != "no_used" and (ok or variant == "mark_below"):
            used[bj] = True
    return matched


def match_reference(gt, pred, thresh):
    """[GT objects, predicted objects, matched GT objects] of one image: what mgu_match_objects adds to its totals"""
    return [len(gt), len(pred), match_variant(gt, pred, thresh)]


def _far(k):
    """a box no case's boxes overlap, and no other _far box"""
    return [1000 + 10 * k, 1000, 1004 + 10 * k, 1004]


def _filled(n, placed, cls=1):
    """n GT objects of class cls: `placed` {index: box}, every other index a box nothing overlaps"""
    return [(cls, list(placed[k]) if k in placed else _far(k)) for k in range(n)]


def _tie(i, j):
    # p0 meets GT i and GT j at IoU 8 / 32 each; p1 is GT j's box
    return dict(gt=_filled(max(i, j) + 1, {i: [0, 0, 4, 4], j: [6, 0, 10, 4]}), pred=[(1, [2, 0, 8, 4]), (1, [6, 0, 10, 4])], thresh=0.25,
                matched=2)


def _threshold(gt_box, pred_box, value, above):
    return dict(gt=[(1, gt_box)], pred=[(1, pred_box)], thresh=math.nextafter(value, 1.0) if above else value, matched=0 if above else 1)


# name -> gt, pred, thresh and the matched count a correct matcher gives, worked out by hand
MATCH_CASES = {
    "tie_3_70": _tie(3, 70),    # different lanes, different strides
    "tie_3_67": _tie(3, 67),    # the same lane
    "tie_9_70": _tie(9, 70),    # the smaller index in the higher lane
    # p0 [0,0,10,10] meets GT 0 at 40/100 and GT 100 at 60/100; p1 meets GT 0 alone, at 16/40
    "larger_beats_earlier": dict(gt=_filled(101, {0: [0, 0, 4, 10], 100: [0, 0, 10, 6]}), pred=[(1, [0, 0, 10, 10]), (1, [0, 6, 4, 10])],
                                 thresh=0.3, matched=2),
    # three times p [0,0,10,10]: GT 70 at 0.8, GT 130 at 0.6, then nothing is left
    "used_persists": dict(gt=_filled(131, {70: [0, 0, 10, 8], 130: [0, 0, 10, 6]}), pred=[(1, [0, 0, 10, 10])] * 3, thresh=0.5, matched=2),
    "half_at": _threshold([0, 0, 4, 4], [0, 0, 4, 2], 0.5, False),
    "half_above": _threshold([0, 0, 4, 4], [0, 0, 4, 2], 0.5, True),
    "third_at": _threshold([0, 0, 3, 1], [0, 0, 1, 1], 1 / 3, False),
    "third_above": _threshold([0, 0, 3, 1], [0, 0, 1, 1], 1 / 3, True),
    # GT 0 (class 2) is p0's box, GT 1 (class 1) meets p0 at 0.6; p1 (class 2) meets GT 0 alone, at 0.4
    "class_filter": dict(gt=[(2, [0, 0, 10, 10]), (1, [0, 0, 10, 6])], pred=[(1, [0, 0, 10, 10]), (2, [0, 6, 10, 10])], thresh=0.3, matched=2),
    # the only GT of p0's class stays under the threshold
    "class_filter_none": dict(gt=[(2, [0, 0, 10, 10]), (1, [0, 0, 10, 2])], pred=[(1, [0, 0, 10, 10])], thresh=0.5, matched=0),
    # p0 meets GT 0 at 0.2, p1 at 0.9
    "below_marks_nothing": dict(gt=[(1, [0, 0, 10, 10])], pred=[(1, [0, 0, 10, 2]), (1, [0, 0, 10, 9])], thresh=0.5, matched=1),
    # zero-area boxes on both sides overlap nothing; the one proper pair matches
    "zero_area": dict(gt=[(1, [5, 5, 5, 9]), (1, [2, 2, 6, 2]), (1, [0, 0, 4, 4])], pred=[(1, [3, 3, 3, 3]), (1, [5, 0, 5, 20]), (1, [0, 0, 4, 4])],
                      thresh=0.5, matched=1),
    # areas of 65535^2 (past 2^31: negative in 32 bits) and 65535 * 32768 (just under 2^31): IoU 32768 / 65535 matches, 32767 / 65535 does not
    "large_boxes": dict(gt=[(1, [0, 0, 65535, 65535]), (1, [0, 0, 65535, 65535])], pred=[(1, [0, 0, 65535, 32767]), (1, [0, 0, 65535, 32768])],
                        thresh=0.5, matched=1),
}

# the cases each wrong matcher must change the matched count of
MATCH_MUTANT_CASES = {
    "tie_last": ["tie_3_70", "tie_3_67", "tie_9_70"],
    "tie_lowest_lane": ["tie_9_70"],
    "first_candidate": ["larger_beats_earlier"],
    "no_used": ["used_persists"],
    "strict_threshold": ["half_at", "third_at"],
    "no_class": ["class_filter", "class_filter_none"],
    "mark_below": ["below_marks_nothing"],
}

GT_SIZES = (0, 1, 63, 64, 65, 200)
PRED_SIZES = (0, 1, 65, 300)
MATCH_BATCH = [(65, 300), (0, 5), (200, 0), (1, 65), (64, 1)]   # (G, NP) per image: unequal, one without GT, one without predictions


def lattice_objects(rng, n):
    """n (class, box): corners on the 0..12 lattice (sides 1..5, cut at 12), three classes -- equal IoUs are common"""
    x0, y0 = rng.integers(0, 12, n), rng.integers(0, 12, n)
    x1, y1 = np.minimum(x0 + rng.integers(1, 6, n), 12), np.minimum(y0 + rng.integers(1, 6, n), 12)
    cls = rng.integers(1, 4, n)
    return [(int(c), [int(a), int(b), int(d), int(e)]) for c, a, b, d, e in zip(cls, x0, y0, x1, y1)]


@functools.lru_cache(maxsize=None)
def lattice_case(G, NP):
    rng = np.random.default_rng(1000 * G + NP)
    return lattice_objects(rng, G), lattice_objects(rng, NP)


def tables(images):
    """(offsets int64 (B + 1), class int64 (N), bbox int32 (N, 4)) of a list of per-image object lists"""
    offsets = np.concatenate([[0], np.cumsum([len(objs) for objs in images])]).astype(np.int64)
    cls = np.array([c for objs in images for c, _ in objs], np.int64)
    bbox = np.array([b for objs in images for _, b in objs], np.int32).reshape(-1, 4)
    return offsets, cls, bbox


def as_dicts(objs):
    """the object lists mgunet.yield_estimation_metrics takes"""
    return [{"bbox": list(b), "class_id": c} for c, b in objs]
