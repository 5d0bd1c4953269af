"""The oracle of the mask input / output kernels (tests/maskio_oracle.py) against independent statements, on the CPU: the outline
properties (a)-(d) of INTEGRATION.md section Y on random masks with scipy.ndimage.label, the fill against matplotlib's point-in-path
test on polygons in general position, COCO's string codec (mgunet.rle_to_string / rle_from_string) by round trip and on a vector
worked by hand -- and the proof that the named cases of tests/maskio_cases.py see the mistakes they are there for: every mutant of
the oracle fails one."""
import numpy as np
import pytest

import maskio_cases as MC
import maskio_oracle as MO
from mgunet import maskio

CASES = MC.label_cases()
FILLS = MC.fill_cases()


def clean(case):
    """the label map with the pixels of no object set to 0"""
    lab = case["labels"].copy()
    n = np.diff(case["offsets"])[:, None, None]
    lab[(lab < 1) | (lab > n)] = 0
    return lab


def small_masks():
    rng = np.random.default_rng(7)
    for k in range(120):
        H, W = rng.integers(1, 11, 2)
        yield (rng.random((H, W)) < (0.3, 0.5, 0.7)[k % 3]).astype(np.int32)


def test_outline_properties_a_to_d_on_random_masks():
    """(a) sum of area2 = 2 * pixels, (b) loops = pieces + holes, (c) positive loops = pieces, (d) the fill of the loops is the mask"""
    ndi = pytest.importorskip("scipy.ndimage")
    full = np.ones((3, 3), int)
    cross = ndi.generate_binary_structure(2, 1)
    loops_seen = late_start = 0
    for m in small_masks():
        if not m.any():
            continue
        H, W = m.shape
        off = np.array([0, 1], np.int64)
        for c in (1, 2):
            lp, vp, v, a2 = MO.outlines(m[None], off, c)
            pieces = ndi.label(m, structure=cross if c == 1 else full)[1]
            holes = ndi.label(np.pad(1 - m, 1, constant_values=1), structure=full if c == 1 else cross)[1] - 1
            assert int(a2.sum()) == 2 * int(m.sum())
            assert len(a2) == pieces + holes, (m, c)
            assert int((a2 > 0).sum()) == pieces and int((a2 < 0).sum()) == holes
            assert np.array_equal(MO.fill(lp, vp, v, off, 1, H, W)[0], m)
            assert (np.diff(vp) >= 4).all() and v.min() >= 0 and v[:, 0].max() <= W and v[:, 1].max() <= H
            loops_seen += len(a2)
            mlp, mvp, mv, _ = MO.outlines(m[None], off, c, mutant_start_at_leader=True)
            late_start += int((np.diff(mvp) != np.diff(vp)).sum())
    assert loops_seen > 500 and late_start > 5      # loops whose leader's start point is no corner do occur


def test_runs_are_maximal_ordered_and_decode_to_the_map():
    for name, case in CASES.items():
        lab, off = case["labels"], case["offsets"]
        B, H, W = lab.shape
        ptr, start, length = MO.encode(lab, off)
        assert len(ptr) == off[-1] + 1
        for i in range(len(ptr) - 1):
            s, n = start[ptr[i]:ptr[i + 1]].astype(np.int64), length[ptr[i]:ptr[i + 1]].astype(np.int64)
            assert (n >= 1).all() and (s[1:] > (s + n)[:-1]).all(), name
            counts = MO.coco_counts(s, n, H * W)
            assert sum(counts) == H * W and all(c > 0 for c in counts[1:]), name
        got, status = MO.decode(ptr, start, length, off, B, H, W)
        assert status == 0 and np.array_equal(got, clean(case)), name
        assert int(length.sum()) == int((clean(case) > 0).sum()), name


def test_full_frame_and_single_pixel_in_closed_form():
    case = CASES["scene_7x5_b3"]
    ptr, start, length = MO.encode(case["labels"], case["offsets"])
    assert (start[-1], length[-1]) == (0, 35) and ptr[-1] - ptr[-2] == 1          # the full frame: one run [0, H*W)
    lp, vp, v, a2 = MO.outlines(case["labels"], case["offsets"], 2)
    assert v[vp[-2]:].tolist() == [[0, 0], [5, 0], [5, 7], [0, 7]] and a2[-1] == 70  # one loop of 4 corners, clockwise on the screen
    one = MC.batch([MC.every_pixel(7, 5)], 1)
    lp, vp, v, a2 = MO.outlines(one["labels"], one["offsets"], 1)
    assert len(a2) == 35 and len(v) == 4 * 35 and (a2 == 2).all()                    # the default capacities are reached exactly


def test_outlines_fill_back_to_every_case():
    for name, case in CASES.items():
        lab, off, c = case["labels"], case["offsets"], case["connectivity"]
        if lab.size > 3000:
            continue            # the sequential oracle fill is per pixel and edge: the large cases run on the GPU
        B, H, W = lab.shape
        lp, vp, v, a2 = MO.outlines(lab, off, c)
        assert np.array_equal(MO.fill(lp, vp, v, off, B, H, W), clean(case)), name
        area = np.array([int(m.sum()) for _, _, m in MO.object_masks(lab, off)], np.int64)
        assert np.array_equal(np.add.reduceat(np.concatenate((a2, [0])), lp[:-1])[:len(area)] * (np.diff(lp) > 0), 2 * area), name


def test_fill_against_matplotlib_in_general_position():
    """polygons that do not cross themselves (star-shaped around a point: matplotlib's non-zero winding equals even-odd), vertices at odd
    sixteenths (never at a centre's height); a centre that an edge passes through is left out of the comparison"""
    path = pytest.importorskip("matplotlib.path")
    rng = np.random.default_rng(3)
    H, W, f = 12, 14, 4
    yy, xx = np.mgrid[0:H, 0:W]
    centres = np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], 1)
    compared = 0
    for _ in range(40):
        n = int(rng.integers(3, 9))
        ang = np.sort(rng.random(n)) * 2 * np.pi
        rad = rng.uniform(1.0, 9.0, n)
        c = rng.uniform(-2.0, 14.0, 2)
        fixed = np.rint(np.stack([c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)], 1) * 8).astype(np.int64) * 2 + 1
        if np.ptp(ang) < np.pi or np.diff(np.concatenate((ang, [ang[0] + 2 * np.pi]))).max() > np.pi * 0.95:
            continue                                   # not star-shaped around c for sure: skip
        inside = path.Path(np.vstack([fixed, fixed[:1]]) / 16.0, closed=True).contains_points(centres)
        got = MO.loops_cover([fixed], H, W, f).ravel()
        clear = ~_centres_near_edges(fixed, centres * 16)
        assert np.array_equal(got[clear], inside[clear])
        compared += int(got[clear].sum())
    assert compared > 300
    tri = np.array([[1, 1], [200, 17], [33, 150]], np.int64)
    assert np.array_equal(MO.loops_cover([tri], H, W, f).ravel(), path.Path(tri / 16.0).contains_points(centres))


def _centres_near_edges(v, pts):
    near = np.zeros(len(pts), bool)
    for j in range(len(v)):
        a, b = v[j].astype(float), v[(j + 1) % len(v)].astype(float)
        t = np.clip(((pts - a) @ (b - a)) / max(float((b - a) @ (b - a)), 1e-12), 0, 1)
        near |= np.linalg.norm(pts - (a + t[:, None] * (b - a)), axis=1) < 1e-6
    return near


def test_fill_cases_hold_what_their_names_say():
    got = {name: MO.fill(*MC.fill_table(c)) for name, c in FILLS.items()}
    lower, upper = got["centre_on_slope"][0] == 1, got["centre_on_slope"][0] == 2
    assert (lower | upper).all() and np.array_equal(upper, np.triu(np.ones((6, 6), bool), 1))\
        and not (lower & upper).any()   # a centre on the diagonal: the crossing is not left of it, so the left edge alone counts -> label 1
    assert int((got["centre_on_vertex"] > 0).sum()) == 18                       # |x - 3| + |y - 3| <= 3 without the upper / right rim
    assert np.array_equal(got["centre_on_vertical"][0] > 0, np.pad(np.ones((2, 3), bool), ((1, 2), (2, 1))))   # rows 1-2: the top rim is in, the bottom out; columns 2-4: the right rim is in
    star = got["star"][0] > 0
    assert not star[10, 10] and star[2, 10] and star.sum() > 40                 # even-odd: the pentagon in the middle is outside
    out = got["outside"][0]
    assert set(np.unique(out)) == {0, 3, 4, 5} and out[0, 0] == 3 and out[7, 9] == 5 and out[5, 2] == 4
    ov = got["overlap"]
    assert ov[0, 4, 4] == 2 and ov[0, 5, 4] == 3 and ov[0, 1, 1] == 1 and not ov[1].any() and set(np.unique(ov[2])) == {0, 2}
    hi = got["hole_and_island"][0]
    assert hi[0, 0] == 1 and hi[3, 3] == 0 and hi[4, 4] == 1 and hi.sum() == 81 - 25 + 1
    dg = got["degenerate_loops"][0]
    assert np.array_equal(dg > 0, np.pad(np.ones((3, 4), bool), ((1, 3), (2, 1)))) and dg.max() == 1
    assert maskio._crossings(*[MC.fill_table(FILLS["tall_65x70"])[k] for k in (2, 1)], 65, 2) > 150


def test_crossing_count_of_the_python_default_is_the_number_of_counted_edges():
    for name, c in FILLS.items():
        lp, vp, v, off, B, H, W, f = MC.fill_table(c)
        S, n = 1 << f, 0
        cy = (2 * np.arange(H) + 1) * S
        for l in range(len(vp) - 1):
            y = 2 * v[vp[l]:vp[l + 1], 1].astype(np.int64)
            for j in range(len(y)):
                n += int(((y[j] <= cy) != (y[(j + 1) % len(y)] <= cy)).sum())
        assert maskio._crossings(v, vp, H, f) == n, name


def test_string_codec_round_trip_and_a_vector_worked_by_hand():
    """[6, 1, 40, 4, 5, 4, 5, 4, 21] by hand: 6 -> '6'; 1 -> '1'; 40 = 8 + 32*1 -> (8 | 0x20) + 48 = 'X', then 1 -> '1'; from the fourth
    count on the difference from two before: 4 - 1 = 3 -> '3'; 5 - 40 = -35 -> low 5 bits 29, rest -2, bit 0x10 set and rest != -1 so
    more: (29 | 0x20) + 48 = 'm', then -2 -> low bits 30, rest -1, sign bit set and rest == -1: done, 30 + 48 = 'N'; 4 - 4, 5 - 5,
    4 - 4 -> '0' each; 21 - 5 = 16 -> low bits 16 with bit 0x10 set and rest 0 != -1 so more: (16 | 0x20) + 48 = '`', then 0 -> '0'."""
    counts = [6, 1, 40, 4, 5, 4, 5, 4, 21]
    assert maskio.rle_to_string(counts) == "61X13mN000`0"
    assert maskio.rle_from_string("61X13mN000`0") == counts
    rng = np.random.default_rng(11)
    for _ in range(200):
        c = rng.integers(0, int(rng.choice([3, 40, 5000, 2 ** 30])), int(rng.integers(1, 30))).tolist()
        s = maskio.rle_to_string(c)
        assert maskio.rle_from_string(s) == c and all(48 <= ord(ch) < 112 for ch in s)
    for name in ("comb", "rings_c1", "scene_7x5_b3"):
        lab, off = CASES[name]["labels"], CASES[name]["offsets"]
        ptr, start, length = MO.encode(lab, off)
        for i in range(len(ptr) - 1):
            counts = MO.coco_counts(start[ptr[i]:ptr[i + 1]], length[ptr[i]:ptr[i + 1]], lab.shape[1] * lab.shape[2])
            assert maskio.rle_from_string(maskio.rle_to_string(counts)) == counts
    with pytest.raises(ValueError):
        maskio.rle_from_string("X")


def runs_differ(name, **mutant):
    c = CASES[name]
    return any(not np.array_equal(a, b) for a, b in zip(MO.encode(c["labels"], c["offsets"]), MO.encode(c["labels"], c["offsets"], **mutant)))


def outlines_differ(name, **mutant):
    c = CASES[name]
    a, b = MO.outlines(c["labels"], c["offsets"], c["connectivity"]), MO.outlines(c["labels"], c["offsets"], c["connectivity"], **mutant)
    return any(not np.array_equal(u, v) for u, v in zip(a, b))


def fills_differ(name, **mutant):
    t = MC.fill_table(FILLS[name])
    return not np.array_equal(MO.fill(*t), MO.fill(*t, **mutant))


def test_every_mutant_fails_a_named_case():
    assert runs_differ("comb", mutant_row_major=True)                       # row-major instead of column-major order
    assert runs_differ("comb", mutant_no_wrap=True)                         # runs not joined across the column wrap
    assert runs_differ("comb_70x3", mutant_no_wrap=True)
    assert outlines_differ("diagonal_c1", mutant_wrong_turn=True)           # the wrong turn at a diagonal touch, each connectivity
    assert outlines_differ("diagonal_c2", mutant_wrong_turn=True)
    assert fills_differ("centre_on_vertical", mutant_strict=True)           # < for <= in the half-open rule: the rim rows swap
    assert fills_differ("overlap", mutant_smallest_wins=True)               # the smallest label instead of the largest
    lab = np.zeros((1, 2, 6), np.int32)
    over = (np.array([0, 1, 2], np.int64), np.array([0, 4], np.int32), np.array([8, 6], np.int32), np.array([0, 2], np.int64), 1, 2, 6)
    assert not np.array_equal(MO.decode(*over)[0], MO.decode(*over, mutant_smallest_wins=True)[0]) and lab.shape
    assert outlines_differ("rings_c1", mutant_start_at_leader=True)         # a loop started at the leader's start point, no corner
    assert outlines_differ("rings_one_object", mutant_start_at_leader=True)
    assert not outlines_differ("cross", mutant_start_at_leader=True)        # outer loops only: their leader is a corner
