"""Named cases for the mask input / output kernels (csrc/maskio.hip): label maps at the sizes and scenes where each piece can go wrong,
and polygon sets for the fill.  Pure numpy; shared by tests/test_maskio_host.py (the oracle against independent statements, the
mutants) and tests/test_gpu_maskio.py (the kernels against the oracle).

A label case is {"labels": int32 (B, H, W), "offsets": int64 (B + 1), "connectivity": 1 or 2}; a fill case is {"polygons": per image
a list of objects, an object a list of loops, a loop a list of (x, y) in pixel units, "size": (H, W), "frac_bits": f}."""
import functools

import numpy as np

SIZES = [(1, 1), (1, 70), (70, 1), (7, 5), (64, 64), (65, 63), (130, 67)]


def label_components(mask, connectivity):
    """int32 labels 1..n of the components of a bool mask, in raster order of their first pixel (a flood fill written out)"""
    H, W = mask.shape
    lab, n = np.zeros((H, W), np.int32), 0
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 2 else [])
    for y0, x0 in np.argwhere(mask):
        if lab[y0, x0]:
            continue
        n += 1
        lab[y0, x0] = n
        todo = [(y0, x0)]
        while todo:
            y, x = todo.pop()
            for dy, dx in steps:
                v, u = y + dy, x + dx
                if 0 <= v < H and 0 <= u < W and mask[v, u] and not lab[v, u]:
                    lab[v, u] = n
                    todo.append((v, u))
    return lab, n


def batch(maps, connectivity):
    """a label case from per-image (labels, n) pairs"""
    labels = np.stack([m for m, _ in maps]).astype(np.int32)
    offsets = np.concatenate(([0], np.cumsum([n for _, n in maps]))).astype(np.int64)
    return {"labels": labels, "offsets": offsets, "connectivity": connectivity}


def random_map(H, W, density, connectivity, seed):
    return label_components(np.random.default_rng(seed).random((H, W)) < density, connectivity)


def checkerboard(H, W, connectivity):
    yy, xx = np.mgrid[0:H, 0:W]
    return label_components((yy + xx) % 2 == 0, connectivity)


def every_pixel(H, W):
    return np.arange(1, H * W + 1, dtype=np.int32).reshape(H, W), H * W


def full_frame(H, W):
    return np.ones((H, W), np.int32), 1


def empty(H, W):
    return np.zeros((H, W), np.int32), 0


def rings(connectivity=None):
    """11 x 11: a ring, inside it a ring, inside that an island.  connectivity None: all three carry label 1 (one object in three
    pieces with two holes), else they are labelled apart."""
    m = np.zeros((11, 11), bool)
    for r in (0, 2, 4):
        m[r:11 - r, r:11 - r] = True
        m[r + 1:10 - r, r + 1:10 - r] = False
    m[5, 5] = True
    return (m.astype(np.int32), 1) if connectivity is None else label_components(m, connectivity)


def diagonal():
    """3 x 4: two pixels of one object that meet only at a corner, and a second object beside them"""
    lab = np.zeros((3, 4), np.int32)
    lab[0, 0] = lab[1, 1] = 1
    lab[2, 3] = 2
    return lab, 2


def comb(H=5, W=7):
    """a spine along the top row with teeth in every other column down to the bottom row: the run of a tooth column continues into the
    spine pixel of the next column"""
    lab = np.zeros((H, W), np.int32)
    lab[0, :] = 1
    lab[:, 0::2] = 1
    return lab, 1


def cross(H=6, W=9):
    """an object cut by all four frame sides, with a second object in one quadrant"""
    lab = np.zeros((H, W), np.int32)
    lab[H // 2, :] = 1
    lab[:, W // 2] = 1
    lab[0, 0:2] = 2
    return lab, 2


def stray_labels():
    """what split_objects with min_area leaves behind: labels outside [1, n_b] (5, 9 and a negative one) belong to no object"""
    lab = np.array([[1, 1, 0, 5, 5], [0, 1, 0, 5, 2], [9, 0, -3, 2, 2], [9, 0, 0, 0, 2]], np.int32)
    return lab, 2


@functools.lru_cache(maxsize=None)
def label_cases():
    cases = {}
    for H, W in SIZES:
        scene = random_map(H, W, 0.5, 2, 100 * H + W)
        cases[f"scene_{H}x{W}_b1"] = batch([scene], 2)
        cases[f"scene_{H}x{W}_b3"] = batch([scene, empty(H, W), full_frame(H, W)], 2)
    for c in (1, 2):
        cases[f"checkerboard_c{c}"] = batch([checkerboard(7, 5, c)], c)
        cases[f"checkerboard_65x63_c{c}"] = batch([checkerboard(65, 63, c)], c)
        cases[f"rings_c{c}"] = batch([rings(c)], c)
        cases[f"diagonal_c{c}"] = batch([diagonal()], c)
    cases["every_pixel_7x5"] = batch([every_pixel(7, 5), every_pixel(7, 5)], 1)
    cases["every_pixel_65x63"] = batch([every_pixel(65, 63)], 2)
    cases["rings_one_object"] = batch([rings(None)], 2)
    cases["comb"] = batch([comb()], 2)
    cases["comb_70x3"] = batch([comb(70, 3), empty(70, 3)], 1)
    cases["cross"] = batch([cross()], 1)
    cases["stray_labels"] = batch([stray_labels(), empty(4, 5), stray_labels()], 2)
    for d in (0.1, 0.5, 0.9):
        for c in (1, 2):
            cases[f"random_d{d}_c{c}"] = batch([random_map(33, 47, d, c, int(d * 10) + c), random_map(33, 47, d, c, 50 + int(d * 10) + c)], c)
    return cases


def star(cx, cy, r, points=5):
    """a pentagram: every second point of a regular polygon, so the loop crosses itself"""
    a = np.pi / 2 + 2 * np.pi * 2 * np.arange(points) / points
    return [(cx + r * np.cos(t), cy - r * np.sin(t)) for t in a]


@functools.lru_cache(maxsize=None)
def fill_cases():
    sq = lambda x0, y0, x1, y1: [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]  # noqa: E731
    return {
        "frac1_halves": {"polygons": [[[[(0.5, 0.5), (6.5, 1.0), (5.0, 6.5), (1.5, 4.0)]]]], "size": (8, 8), "frac_bits": 1},
        "frac4_sixteenths": {"polygons": [[[[(1.0625, 0.9375), (9.4375, 2.5), (7.8125, 8.0625), (0.3125, 6.6875)]]]], "size": (9, 11), "frac_bits": 4},
        # the diagonal (0,0)-(6,6) runs through the centres (k + 1/2, k + 1/2)
        "centre_on_slope": {"polygons": [[[[(0, 0), (6, 6), (0, 6)]], [[(0, 0), (6, 0), (6, 6)]]]], "size": (6, 6), "frac_bits": 0},
        # a diamond whose four vertices are pixel centres
        "centre_on_vertex": {"polygons": [[[[(3.5, 0.5), (6.5, 3.5), (3.5, 6.5), (0.5, 3.5)]]]], "size": (7, 7), "frac_bits": 1},
        # vertical edges through the centres of columns 1 and 4, horizontal ones through the centres of rows 1 and 3
        "centre_on_vertical": {"polygons": [[[sq(1.5, 1.5, 4.5, 3.5)]]], "size": (5, 6), "frac_bits": 1},
        "star": {"polygons": [[[star(10.0, 10.5, 9.7)]]], "size": (21, 20), "frac_bits": 4},
        "outside": {"polygons": [[[sq(-9, -9, -2, -3)], [sq(20, 2, 30, 5)], [sq(-3, -2, 4, 3)], [[(-5, 3), (15, 2), (4, 30)]], [sq(5, 4, 40, 40)]]],
                    "size": (8, 10), "frac_bits": 0},
        "overlap": {"polygons": [[[sq(1, 1, 6, 6)], [sq(4, 3, 9, 8)], [sq(0, 5, 5, 9)]], [], [[sq(2, 2, 5, 5)], [sq(2, 2, 5, 5)]]],
                    "size": (9, 10), "frac_bits": 0},
        "hole_and_island": {"polygons": [[[sq(0, 0, 9, 9), sq(2, 2, 7, 7)[::-1], sq(4, 4, 5, 5)]]], "size": (9, 9), "frac_bits": 0},
        "degenerate_loops": {"polygons": [[[[(1, 1), (5, 6)], [], sq(2, 1, 6, 4), [(3, 3)]], [[], []]]], "size": (7, 7), "frac_bits": 0},
        "tall_65x70": {"polygons": [[[[(3.25, -4.0), (60.5, 10.75), (33.0, 80.0)]], [star(35.0, 32.5, 30.3)]]], "size": (65, 70), "frac_bits": 2},
    }


def fill_table(case):
    """(loop_ptr, vertex_ptr, vertices, offsets, B, H, W, frac_bits) of a fill case, for maskio_oracle.fill and the raw call"""
    import maskio_oracle as MO
    lp, vp, v, off = MO.polygon_table(case["polygons"], case["frac_bits"])
    return lp, vp, v, off, len(case["polygons"]), case["size"][0], case["size"][1], case["frac_bits"]
