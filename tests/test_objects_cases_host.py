"""CPU tier of the designed object cases (tests/objects_cases.py): every labelling scene has the property it is there for, the numpy
oracle equals scipy.ndimage.label on all of them, every restated wrong kernel differs from the oracle on the scenes designated for
it, every restated wrong matcher changes the matched count of its designated cases, and the matching reference agrees with
mgunet.objects._match_host.  No GPU needed; tests/test_gpu_objects_scenes.py and tests/test_gpu_match_objects.py run the same cases
on the device."""
import numpy as np
import pytest

import objects_cases as OC
import objects_oracle as OO
from mgunet import objects as mobj

T = OC.TILE


def ncomp(m, connectivity):
    return int(OO.label(m, connectivity).max(initial=0))


# ---- scene properties -------------------------------------------------------------------------------------------------------------
def test_constants_follow_the_kernel_file():
    import os
    import re
    src = open(os.path.join(os.path.dirname(mobj.__file__), "..", "csrc", "objects.hip")).read()
    assert int(re.search(r"constexpr int TILE = (\d+);", src).group(1)) == OC.TILE
    threads = int(re.search(r"constexpr int OB_THREADS = (\d+);", src).group(1))
    assert re.search(r"constexpr int CHUNK = 4 \* OB_THREADS;", src) and 4 * threads == OC.CHUNK
    assert "lane == (int)(bj % 64)" in src and OC.LANES == 64
    hdr = open(os.path.join(os.path.dirname(mobj.__file__), "..", "csrc", "objects_common.h")).read()
    assert int(re.search(r"constexpr int SCAN_THREADS = (\d+);", hdr).group(1)) == OC.SCAN_THREADS


@pytest.mark.parametrize("size", OC.SIZES)
@pytest.mark.parametrize("name", list(OC.PATHS))
def test_paths_are_one_component(name, size):
    m = OC.scene(name, size)
    for connectivity in (1, 2):
        assert ncomp(m, connectivity) == 1, connectivity
    H, W = size
    if name == "row_serpentine":     # one joining pixel between two full rows, at alternating ends
        assert m[0::2].all() and (m[1::2].sum(1) == 1).all()
        assert m[1::4, W - 1].all() and m[3::4, 0].all()
    elif name == "col_serpentine":   # one joining pixel between two bars: bar k meets bar k - 1 only in its last or first row
        assert m[:, 0::2].all() and (m[:, 1::2].sum(0) == 1).all()
        assert m[H - 1, 1::4].all() and m[0, 3::4].all()
    elif name == "comb":
        assert m[H - 1].all() and m[:H - 1, 0::2].all() and not m[:H - 1, 1::2].any()
        assert ncomp(m[:H - 1], 2) == (W + 1) // 2                  # without the last row every tooth stands alone
    else:                            # the spiral never touches itself: its complement is one spiral too, and it is a path
        assert ncomp(1 - m, 1) == 1
        y, x = np.nonzero(m)
        deg = sum(np.pad(m, 1)[1 + y + dy, 1 + x + dx] for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)))
        assert np.bincount(deg).tolist() == [0, 2, len(y) - 2]  # two ends, every other pixel has two neighbours
        assert len(y) > H * W // 2 - H - W
    c = OC.scene(name + "_compl", size)
    assert np.array_equal(c == 1, m == 1) and np.array_equal(c == 2, m == 0)
    for connectivity in (1, 2):      # nothing joins across the two classes
        assert ncomp(c, connectivity) == 1 + ncomp(1 - m, connectivity)


@pytest.mark.parametrize("size", OC.SIZES)
def test_rings_are_nested(size):
    H, W = size
    m = OC.scene("rings", size)
    n = (min(H, W) + 3) // 4         # rings at insets 0, 2, 4, ...; the innermost may be a bar or a point
    assert ncomp(m, 1) == n and ncomp(m, 2) == n
    assert m[0].all() and not m[1, 1:W - 1].any() and m[2, 2:W - 2].all()
    assert ncomp(OC.scene("rings_compl", size), 2) == n + ncomp(1 - m, 2)


@pytest.mark.parametrize("size", OC.SIZES)
def test_diagonals_pass_through_or_beside_tile_corners(size):
    H, W = size
    main, anti = OC.scene("diag_main", size), OC.scene("diag_anti", size)
    s = OC.anti_sum(H)
    on_main = [(cy, cx) for cy, cx in OC.tile_corners(H, W) if cy == cx]
    on_anti = [(cy, cx) for cy, cx in OC.tile_corners(H, W) if cy + cx == s + 1]
    assert len(on_main) >= 1 and len(on_anti) >= 1
    for cy, cx in on_main:           # only the NW and the SE pixel of the corner's 2 x 2 block
        assert main[cy - 1:cy + 1, cx - 1:cx + 1].tolist() == [[1, 0], [0, 1]]
    for cy, cx in on_anti:           # only the NE and the SW pixel
        assert anti[cy - 1:cy + 1, cx - 1:cx + 1].tolist() == [[0, 1], [1, 0]]
    for name, line in (("diag_main", main), ("diag_anti", anti), ("diag_main_shift", OC.scene("diag_main_shift", size)),
                       ("diag_anti_shift", OC.scene("diag_anti_shift", size))):
        assert ncomp(line, 1) == int(line.sum()) and ncomp(line, 2) == 1, name   # 4-neighbours: every pixel alone; 8: one line
    ms, as_ = OC.scene("diag_main_shift", size), OC.scene("diag_anti_shift", size)
    for cy, cx in on_main:           # one column on: the line crosses a vertical and a horizontal tile edge beside the corner
        assert ms[cy - 1:cy + 1, cx - 1:cx + 2].tolist() == [[0, 1, 0], [0, 0, 1]] and ms[cy - 2, cx - 1] == 1
    for cy, cx in on_anti:
        assert as_[cy - 1:cy + 1, cx - 1:cx + 2].tolist() == [[0, 0, 1], [0, 1, 0]] and as_[cy + 1, cx - 1] == 1
    x = OC.scene("diag_x", size)
    assert np.array_equal(x, main | anti) and ncomp(x, 1) <= int(x.sum())
    if size == (96, 96):             # the two lines cross between pixels: their four middle pixels form one 2 x 2 block
        assert int(main.sum()) == 96 and int(anti.sum()) == 96 and ncomp(x, 2) == 1 and ncomp(x, 1) == 192 - 3


@pytest.mark.parametrize("size", OC.SIZES)
@pytest.mark.parametrize("kind", ["nwse", "nesw"])
def test_corner_contacts_join_through_the_diagonal_tile_alone(kind, size):
    m = OC.scene("corner_" + kind, size)
    corners = OC.tile_corners(*size)
    assert len(corners) >= 2 and int(m.sum()) == 2 * len(corners)
    assert ncomp(m, 1) == 2 * len(corners) and ncomp(m, 2) == len(corners)
    ys, xs = np.nonzero(m)
    tiles = {(cy, cx): set() for cy, cx in corners}
    for y, x in zip(ys, xs):
        tiles[(T * ((y + 1) // T), T * ((x + 1) // T))].add((y // T, x // T))
    for (cy, cx), ts in tiles.items():   # the two pixels of a corner lie in diagonally adjacent tiles
        (a, b), (c, d) = sorted(ts)
        assert abs(a - c) == 1 and abs(b - d) == 1


@pytest.mark.parametrize("size", OC.SIZES)
@pytest.mark.parametrize("kind", ["h", "v"])
def test_edge_contacts_touch_through_one_pixel_pair(kind, size):
    m = OC.scene("edge_" + kind, size)
    assert ncomp(m, 1) == 3 and ncomp(m, 2) == 3
    y, x = np.nonzero(m)
    if kind == "h":                  # pairs across the tile edge between columns 31 and 32
        rows = np.flatnonzero(m[:, T - 1] & m[:, T])
        assert rows.tolist() == [T + p for p in OC.EDGE_POSITIONS]
        cut = m.copy()
        cut[rows, T - 1] = 0
    else:
        c0 = T if size[1] >= 2 * T else 0
        cols = np.flatnonzero(m[2 * T - 1] & m[2 * T])
        assert cols.tolist() == [c0 + p for p in OC.EDGE_POSITIONS]
        cut = m.copy()
        cut[2 * T - 1, cols] = 0
    assert ncomp(cut, 1) == 6        # without the three contact pixels the six rectangles are apart
    assert int(m.sum()) == (3 * (8 + 28) if kind == "h" else 3 * (8 + 16))


def test_area_map_holds_one_rectangle_per_area():
    m = OC.area_map()
    for connectivity in (1, 2):
        lab = OO.label(m, connectivity)
        _, area, bbox, _ = OO.stats(lab, m)
        assert sorted(area.tolist()) == list(OC.AREAS)
        assert np.array_equal((bbox[:, 2] - bbox[:, 0]) * (bbox[:, 3] - bbox[:, 1]), area)   # rectangles
        for k in OC.MIN_AREAS:
            assert int(OO.label(m, connectivity, min_area=k).max(initial=0)) == max(0, 71 - k)
    assert min(OC.MIN_AREAS) == 1 and {63, 64, 65} <= set(OC.MIN_AREAS) and max(OC.MIN_AREAS) == max(OC.AREAS) + 1


def test_large_batches_reach_the_scan_segments():
    assert [OC.scan_segment(*s) for s in OC.LARGE_BATCHES] == [(1025, 2), (2049, 3), (1400, 2)]
    assert all(n % seg or n // seg < OC.SCAN_THREADS for n, seg in map(lambda s: OC.scan_segment(*s), OC.LARGE_BATCHES))   # ragged tails
    assert OC.scan_segment(65535, 1, 1) == (65535, 64)
    maps, labels, counts, offsets = OC.single_pixel_batch()
    assert maps.shape == (65535, 1, 1) and counts.sum() == 32768 and offsets[-1] == 32768 and offsets[2] == 1
    for b in (0, 1, 65534):
        assert np.array_equal(labels[b], OO.label(maps[b], 2))


@pytest.mark.parametrize("connectivity", [1, 2])
def test_stacked_oracle_equals_per_image_oracle(connectivity):
    rng = np.random.default_rng(4)
    maps = (rng.random((40, 3, 5)) < 0.5).astype(np.int64) * rng.integers(1, 3, (40, 3, 5))
    maps[7] = 0
    maps[39] = 0
    labels, counts, offsets, *st = OC.stacked_table(maps, connectivity)
    ref = np.stack([OO.label(m, connectivity) for m in maps])
    rcounts, roffsets, *rst = OC.table_of(ref, maps)
    assert np.array_equal(labels, ref) and np.array_equal(counts, rcounts) and np.array_equal(offsets, roffsets)
    for a, b in zip(st, rst):
        assert np.array_equal(a, b)


# ---- the oracle against scipy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", OC.SIZES)
def test_oracle_equals_scipy_on_every_scene(size):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = {1: ndi.generate_binary_structure(2, 1), 2: np.ones((3, 3), int)}
    maps = [(n, OC.scene(n, size)) for n in OC.SCENE_NAMES] + ([("area_map", OC.area_map())] if size == OC.SIZES[0] else [])
    for name, m in maps:
        for connectivity in (1, 2):
            # scipy labels a binary map: one class at a time, objects then renumbered in raster order of their first pixel
            first, parts = [], []
            for v in np.unique(m[m != 0]):
                lab, n = ndi.label(m == v, structure[connectivity])
                parts.append((lab, n))
                first += [(int(np.flatnonzero(lab.ravel() == k)[0]), len(parts) - 1, k) for k in range(1, n + 1)]
            want = np.zeros(m.shape, np.int32)
            for rank, (_, part, k) in enumerate(sorted(first)):
                want[parts[part][0] == k] = rank + 1
            assert np.array_equal(OO.label(m, connectivity), want), (name, connectivity)


# ---- labelling mutants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", OC.SIZES)
def test_restated_kernel_equals_the_oracle(size):
    for name in OC.SCENE_NAMES:
        for connectivity in (1, 2):
            assert np.array_equal(OC.tiled_label(OC.scene(name, size), connectivity), OC.expected(name, size, connectivity)[0]), (name, connectivity)


@pytest.mark.parametrize("variant", list(OC.LABEL_MUTANT_SCENES))
def test_wrong_border_passes_show_on_their_scenes(variant):
    assert set(OC.LABEL_MUTANT_SCENES) == set(OC.LABEL_VARIANTS) - {"kernel"}
    for name, size, connectivity in OC.LABEL_MUTANT_SCENES[variant]:
        assert not np.array_equal(OC.tiled_label(OC.scene(name, size), connectivity, variant), OC.expected(name, size, connectivity)[0]), (name, size)


@pytest.mark.parametrize("size", OC.SIZES)
def test_numbering_without_the_image_offset_shows_on_the_batch(size):
    ref = np.stack([OC.expected(n, size, 2)[0] for n in OC.SCENE_NAMES])
    wrong = OC.numbered_without_image_offset(ref)
    assert np.array_equal(wrong[0], ref[0]) and all(not np.array_equal(wrong[b], ref[b]) for b in range(1, len(ref)))


# ---- matching ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OC.MATCH_CASES))
def test_match_cases_give_their_hand_count(name):
    c = OC.MATCH_CASES[name]
    assert OC.match_reference(c["gt"], c["pred"], c["thresh"]) == [len(c["gt"]), len(c["pred"]), c["matched"]]


def test_match_cases_hold_the_ious_they_name():
    c = OC.MATCH_CASES
    for name, (i, j) in (("tie_3_70", (3, 70)), ("tie_3_67", (3, 67)), ("tie_9_70", (9, 70))):
        p0, p1 = (b for _, b in c[name]["pred"])
        gt = [b for _, b in c[name]["gt"]]
        assert OC.iou(p0, gt[i]) == OC.iou(p0, gt[j]) == 0.25 and OC.iou(p1, gt[j]) == 1.0 and OC.iou(p1, gt[i]) == 0.0
        assert [k for k, g in enumerate(gt) if OC.iou(p0, g) > 0] == [i, j]
    assert (3 % 64, 70 % 64, 67 % 64, 9 % 64) == (3, 6, 3, 9)             # lanes: different, the same, the smaller index higher
    gt, (p0, p1) = [b for _, b in c["larger_beats_earlier"]["gt"]], [b for _, b in c["larger_beats_earlier"]["pred"]]
    assert (OC.iou(p0, gt[0]), OC.iou(p0, gt[100]), OC.iou(p1, gt[0]), OC.iou(p1, gt[100])) == (0.4, 0.6, 0.4, 0.0)
    gt, p = [b for _, b in c["used_persists"]["gt"]], c["used_persists"]["pred"][0][1]
    assert (OC.iou(p, gt[70]), OC.iou(p, gt[130])) == (0.8, 0.6) and len(c["used_persists"]["pred"]) == 3
    for name, v in (("half", 0.5), ("third", 1 / 3)):
        at, above = c[name + "_at"], c[name + "_above"]
        assert OC.iou(at["pred"][0][1], at["gt"][0][1]) == v == at["thresh"]
        assert above["thresh"] > v and above["thresh"] == np.nextafter(v, 1.0)
    gt, (p0, p1) = c["below_marks_nothing"]["gt"], [b for _, b in c["below_marks_nothing"]["pred"]]
    assert (OC.iou(p0, gt[0][1]), OC.iou(p1, gt[0][1])) == (0.2, 0.9)
    big = c["large_boxes"]
    assert (big["gt"][0][1][2] - big["gt"][0][1][0]) ** 2 > 2 ** 31
    assert [OC.iou(p, big["gt"][0][1]) for _, p in big["pred"]] == [32767 / 65535, 32768 / 65535]


@pytest.mark.parametrize("variant", list(OC.MATCH_MUTANT_CASES))
def test_wrong_matchers_change_their_cases(variant):
    assert set(OC.MATCH_MUTANT_CASES) == set(OC.MATCH_VARIANTS) - {"kernel"}
    for name in OC.MATCH_MUTANT_CASES[variant]:
        c = OC.MATCH_CASES[name]
        assert OC.match_variant(c["gt"], c["pred"], c["thresh"], variant) != c["matched"], name


def test_lowest_lane_matcher_is_right_where_lanes_follow_indices():
    for name in ("tie_3_70", "tie_3_67"):   # why (9, 70) is there: here the lowest lane holds the smallest index
        c = OC.MATCH_CASES[name]
        assert OC.match_variant(c["gt"], c["pred"], c["thresh"], "tie_lowest_lane") == c["matched"]


def _all_match_inputs():
    for name, c in OC.MATCH_CASES.items():
        yield name, c["gt"], c["pred"], c["thresh"]
    for G in OC.GT_SIZES:
        for NP in OC.PRED_SIZES:
            yield (G, NP), *OC.lattice_case(G, NP), 0.5
    for G, NP in OC.MATCH_BATCH:
        yield ("batch", G, NP), *OC.lattice_case(G, NP), 0.3


def test_reference_agrees_with_the_host_matcher():
    for name, gt, pred, thresh in _all_match_inputs():
        n_gt, n_match, _, _ = mobj._match_host([OC.as_dicts(gt)], [OC.as_dicts(pred)], thresh)
        assert [n_gt, len(pred), n_match] == OC.match_reference(gt, pred, thresh), name


def test_lattice_cases_hold_ties_and_matches():
    gt, pred = OC.lattice_case(200, 300)
    ties = sum(1 for _, p in pred[:40] if (lambda v: len(v) != len(set(v)))([OC.iou(p, g) for _, g in gt if OC.iou(p, g) > 0]))
    assert ties >= 20
    assert 0 < OC.match_reference(gt, pred, 0.5)[2] < 200
    assert {c for c, _ in gt} == {1, 2, 3}
    offsets, cls, bbox = OC.tables([OC.lattice_case(G, NP)[0] for G, NP in OC.MATCH_BATCH])
    assert offsets.tolist() == [0, 65, 65, 265, 266, 330] and cls.shape == (330,) and bbox.shape == (330, 4) and bbox.dtype == np.int32
