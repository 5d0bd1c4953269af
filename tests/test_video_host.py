"""The numpy oracle of the video stage (tests/video_oracle.py) against its own definition, on the cases the GPU suite shares
(tests/video_cases.py): surfaces against the definition's triple loop, known shifts recovered with cost 0, each deliberate mistake
shown to differ from the definition on a shared case, links on visible areas, and track ids of a hand-written link table.  No GPU."""
import numpy as np
import pytest

import video_cases as VC
import video_oracle as VO

CASES = VC.registration_cases()


def test_luma_and_coarse_plane():
    px = np.array([[[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]]], np.uint8)
    assert VO.luma(px).tolist() == [[[255, 0, (77 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (29 * 255 + 128) >> 8, (770 + 3000 + 870 + 128) >> 8]]]
    assert VO.luma(px, bgr=True)[0, 0, 2] == (29 * 255 + 128) >> 8
    grey = np.arange(35, dtype=np.uint8).reshape(1, 5, 7)
    assert np.array_equal(VO.luma(grey), grey)
    c = VO.coarse(grey, 2)                                   # the trailing row and column are dropped; (sum + 2) // 4
    assert c.shape == (1, 2, 3) and c[0, 0, 0] == (0 + 1 + 7 + 8 + 2) // 4 and c[0, 1, 2] == (18 + 19 + 25 + 26 + 2) // 4
    assert np.array_equal(VO.coarse(grey, 1), grey)


@pytest.mark.parametrize("name", ["40x56 f1 R3", "grey", "half zero", "f8 smallest"])
def test_surface_equals_the_triple_loop(name):
    frames, R, f, bgr = CASES[name]
    c = VO.coarse(VO.luma(frames, bgr), f)
    _, _, surf = VO.frame_shifts(frames, R, f, bgr)
    for t in range(len(frames) - 1):
        assert np.array_equal(surf[t], VO.brute_surface(c[t], c[t + 1], R)), (name, t)


def test_shifts_equal_a_brute_force_choice():
    frames, R, f, bgr = CASES["T5 bgr"]
    shifts, cost, surf = VO.frame_shifts(frames, R, f, bgr)
    for t in range(4):
        keys = sorted((int(surf[t][sy + R, sx + R]), sy * sy + sx * sx, sy, sx) for sy in range(-R, R + 1) for sx in range(-R, R + 1))
        assert tuple(shifts[t]) == keys[0][2:] and cost[t][0] == keys[0][0] and cost[t][1] == surf[t][R, R]


@pytest.mark.parametrize("name", list(VC.KNOWN))
def test_known_shifts_are_recovered_with_cost_zero(name):
    offsets, H, W, ch, R, f = VC.KNOWN[name]
    frames = VC.crops(100 + f, H, W, offsets, ch)
    shifts, cost, _ = VO.frame_shifts(frames, R, f)
    assert np.array_equal(shifts, VC.true_shifts(offsets)) and not cost[:, 0].any()
    assert all(int(v) % f == 0 for v in VC.true_shifts(offsets).ravel())


def test_special_frames():
    frames, R, f, _ = CASES["uniform"]
    shifts, cost, surf = VO.frame_shifts(frames, R, f)
    assert not shifts.any() and not surf.any() and not cost.any()
    assert not VO.frame_shifts(*CASES["uniform f2"][:3])[0].any()
    frames, R, f, _ = CASES["0 vs 255"]
    shifts, cost, surf = VO.frame_shifts(frames, R, f)
    n = (frames.shape[1] - 2 * R) * (frames.shape[2] - 2 * R)
    assert n >= 128 * 128 and (surf == 255 * n).all() and not shifts.any() and cost.tolist() == [[255 * n, 255 * n]]
    assert 255 * n > 65535 * 16                              # far beyond what a 16-bit partial holds
    frames, R, f, _ = CASES["corner"]
    assert VO.frame_shifts(frames, R, f)[0].tolist() == [[-R, R]]
    frames, R, f, _ = CASES["corner f2"]
    assert VO.frame_shifts(frames, R, f)[0].tolist() == [[2 * R, -2 * R]]
    with pytest.raises(ValueError):
        VO.frame_shifts(np.zeros((2, 23, 40), np.uint8), 8, 1)


def differs(variant, names):
    """the shared cases on which the variant's shifts, costs or surface differ from the definition's"""
    out = []
    for n in names:
        frames, R, f, bgr = CASES[n]
        want, got = VO.frame_shifts(frames, R, f, bgr), VO.frame_shifts(frames, R, f, bgr, variant=variant)
        if any(not np.array_equal(a, b) for a, b in zip(want, got)):
            out.append(n)
    return out


def test_each_wrong_variant_differs_on_a_shared_case():
    assert differs("sign", ["40x56 f1 R3", "67x93 f2 R4"]) == ["40x56 f1 R3", "67x93 f2 R4"]       # the shift sign reversed
    frames, R, f, bgr = CASES["40x56 f1 R3"]
    assert np.array_equal(VO.frame_shifts(frames, R, f, bgr, variant="sign")[0], -VO.frame_shifts(frames, R, f, bgr)[0])
    assert differs("first", ["uniform", "uniform f2"]) == ["uniform", "uniform f2"]                 # first-found ties
    assert VO.frame_shifts(*CASES["uniform"][:3], variant="first")[0].tolist() == [[-4, -4]] * 2
    assert differs("masked", ["0 vs 255", "half zero"]) == ["0 vs 255", "half zero"]                # zero reference bytes skipped
    assert not VO.frame_shifts(*CASES["0 vs 255"][:3], variant="masked")[2].any()
    assert differs("shrunk", ["40x56 f1 R3", "grey"]) == ["40x56 f1 R3", "grey"]                    # the window shrunk per shift


# ---- tracks --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    frames, cls, disc, shifts = VC.track_scene()
    labels, offsets, class_id, area = VO.label_frames(cls)
    return {"frames": frames, "cls": cls, "disc": disc, "shifts": shifts, "labels": labels, "offsets": offsets, "class_id": class_id, "area": area}


def disc_of_objects(s):
    """the disc every object is a view of"""
    out = []
    for t in range(s["labels"].shape[0]):
        for k in range(1, int(s["offsets"][t + 1] - s["offsets"][t]) + 1):
            d = np.unique(s["disc"][t][s["labels"][t] == k])
            assert d.size == 1 and d[0] > 0
            out.append(int(d[0]) - 1)
    return np.asarray(out)


def test_the_scene_registers_exactly(scene):
    shifts, cost, _ = VO.frame_shifts(scene["frames"], VC.TRACK_RADIUS, 1)
    assert np.array_equal(shifts, scene["shifts"]) and not cost[:, 0].any()
    assert len({tuple(s) for s in shifts.tolist()}) == 5                       # every pair moves differently


def test_alignment_and_visible_areas(scene):
    prev, nxt, vp, vn = VO.track_align(scene["labels"], scene["offsets"], scene["shifts"])
    H, W = VC.TRACK_HW
    for b in range(5):
        sy, sx = scene["shifts"][b]
        for y, x in [(0, 0), (H - 1, W - 1), (20, 30), (H - 1, 0)]:
            inside = 0 <= y - sy < H and 0 <= x - sx < W
            assert prev[b, y, x] == (scene["labels"][b, y - sy, x - sx] if inside else 0)
            assert nxt[b, y, x] == (scene["labels"][b + 1, y, x] if inside else 0)
        assert np.array_equal(scene["disc"][b + 1][prev[b] > 0] > 0, np.ones(int((prev[b] > 0).sum()), bool))   # discs land on discs
    assert (vp <= scene["area"]).all() and (vn <= scene["area"]).all() and (vp < scene["area"]).any()


def test_links_follow_the_discs_and_need_visible_areas(scene):
    link = VO.link_objects(scene["labels"], scene["offsets"], scene["class_id"], scene["shifts"], 0.3)
    disc = disc_of_objects(scene)
    frame = np.repeat(np.arange(6), np.diff(scene["offsets"]))
    for i in range(len(link)):
        before = [j for j in range(len(link)) if frame[j] == frame[i] - 1 and disc[j] == disc[i]]
        assert link[i] == (before[0] if before else -1), i
    # disc 6 shows one pixel in frame 3 and whole in frame 4; disc 5 is half visible in frame 2
    one = [i for i in range(len(link)) if disc[i] == 6 and frame[i] == 3]
    assert len(one) == 1 and scene["area"][one[0]] == 1
    half = [i for i in range(len(link)) if disc[i] == 5 and frame[i] == 2][0]
    whole5 = [i for i in range(len(link)) if disc[i] == 5 and frame[i] == 3][0]
    assert 0.35 < scene["area"][half] / scene["area"][whole5] < 0.65 and link[whole5] == half
    wrong = VO.link_objects(scene["labels"], scene["offsets"], scene["class_id"], scene["shifts"], 0.3, variant="whole")
    four = [i for i in range(len(link)) if disc[i] == 6 and frame[i] == 4][0]
    assert link[four] == one[0] and wrong[four] == -1                          # whole areas: IoU 1 / 149, the track breaks
    # the touching discs of two classes stay two tracks
    tid, n, lengths, classes, _ = VO.track_ids(scene["offsets"], link, scene["class_id"])
    assert n == len(set(disc.tolist())) and all(len(set(tid[disc == d].tolist())) == 1 for d in set(disc.tolist()))
    assert {d: lengths[int(tid[disc == d][0])] for d in (2, 3)} == {2: int((disc == 2).sum()), 3: int((disc == 3).sum())}
    assert classes[int(tid[disc == 2][0])] == 1 and classes[int(tid[disc == 3][0])] == 2


def test_score_order_changes_who_links_first():
    """two objects of the next frame over one of the previous: list order gives it to the first, score order to the better scored"""
    lab = np.zeros((2, 8, 12), np.int32)
    lab[0, 2:6, 2:10] = 1
    lab[1, 2:6, 2:6], lab[1, 2:6, 7:10] = 1, 2
    off, cls = np.array([0, 1, 3], np.int64), np.array([1, 1, 1], np.int64)
    z = np.zeros((1, 2), np.int32)
    assert VO.link_objects(lab, off, cls, z, 0.3).tolist() == [-1, 0, -1]
    assert VO.link_objects(lab, off, cls, z, 0.3, scores=np.array([0, 0.2, 0.9], np.float32)).tolist() == [-1, -1, 0]
    assert VO.link_objects(lab, off, np.array([1, 2, 1], np.int64), z, 0.3).tolist() == [-1, -1, 0]      # classes must agree


def test_track_ids_of_a_hand_written_link_table():
    off = np.array([0, 2, 5, 7, 7, 8], np.int64)
    link = np.array([-1, -1, 1, -1, 0, 3, 2, -1], np.int64)
    cls = np.array([1, 2, 2, 1, 1, 1, 2, 2], np.int64)
    tid, n, lengths, classes, st = VO.track_ids(off, link, cls)
    assert tid.tolist() == [0, 1, 1, 2, 0, 2, 1, 3] and n == 4 and st == 0
    assert lengths == {0: 2, 1: 3, 2: 2, 3: 1} and classes == {0: 1, 1: 2, 2: 1, 3: 2}
    # continuation: the second call starts with the first call's last frame and that frame's ids, and does not count it again
    a = VO.track_ids(off[:3], link[:5], cls[:5])
    off2, link2 = off[1:] - off[1], np.concatenate([[-1, -1, -1], np.where(link[5:] >= 0, link[5:] - off[1], -1)])
    b = VO.track_ids(off2, link2, cls[2:], first_ids=a[0][2:5], next_id=a[1])
    assert np.concatenate([a[0], b[0][3:]]).tolist() == tid.tolist() and b[1] == 4
    merged = dict(a[2])
    for k, v in b[2].items():
        merged[k] = merged.get(k, 0) + v
    assert merged == lengths and {**a[3], **b[3]} == classes
    assert VO.track_ids(off, link, cls, capacity=3)[4] == 1 and VO.track_ids(off, link, cls, capacity=4)[4] == 0


# ---- the work splits of frame_sad_kernel: which case reaches which --------------------------------------------------------------------
PATHS = VC.path_cases()
ALL8 = {(p, c, s) for p in ("whole", "word") for c in (False, True) for s in (False, True)}


def table_paths(min_th=1, with_path_cases=True):
    """the union of sad_paths over every case table of the video suite"""
    tables = [CASES.values(), [(VC.crops(100 + f, H, W, o, ch), R, f, False) for o, H, W, ch, R, f in VC.KNOWN.values()],
              [(VC.track_scene()[0], VC.TRACK_RADIUS, 1, False)]]
    if with_path_cases:         # and the other tables that came with them
        tables += [PATHS.values(), VC.low_amplitude_cases().values(), [VC.alternating_columns()],
                   [(VC.tie_frames(p), VC.TIE_RADIUS, 1, False) for p in VC.TIE_SHIFTS]]
    return set().union(*(VC.case_paths(fr, R, f, min_th) for t in tables for fr, R, f, _ in t))


def test_the_mirror_of_the_work_split():
    assert VC.sad_split(8) == (17, 5, 17) and VC.sad_split(13) == (27, 8, 27) and VC.sad_split(14) == (29, 8, 29)     # 232 tasks: the last unchunked
    assert VC.sad_split(15) == (31, 9, 28) and VC.sad_split(16) == (33, 9, 28) and VC.sad_split(32) == (65, 17, 15)
    assert VC.sad_workgroups(79, 127, 15, 15) == {(48, 48, 28, 1), (48, 48, 3, 9), (1, 48, 28, 1), (1, 48, 3, 1), (48, 1, 28, 1), (48, 1, 3, 9),
                                                  (1, 1, 28, 1), (1, 1, 3, 1)}
    assert VC.sad_workgroups(40, 56, 3, 3) == {(34, 48, 7, 12), (34, 2, 7, 12)}
    assert VC.levels(67, 93, 4, 2) == [(33, 46, 4, 4), (67, 93, 10, 2)]


def test_the_case_tables_reach_every_work_split():
    got = table_paths()
    assert {k[:3] for k in got} == ALL8
    assert {k[3] for k in got if k[0] == "word"} == {0, 1, 2, 3} and {k[3] for k in got if k[0] == "whole"} == {0}
    # whole rows with S = 1 on a tile of at least two rows (a one-row tile has S = 1 whatever the split)
    assert {("whole", False, False, 0), ("whole", True, False, 0)} <= table_paths(min_th=2)
    # the tables before path_cases(): no chunked whole-row tile, and whole rows with S = 1 on one-row tiles only
    old = table_paths(with_path_cases=False)
    assert not [k for k in old if k[0] == "whole" and k[1]] and ("whole", False, False, 0) in old
    assert ("whole", False, False, 0) not in table_paths(min_th=2, with_path_cases=False)
    # what each new case is there for
    paths = {n: VC.case_paths(fr, R, f, min_th=2) for n, (fr, R, f, _) in PATHS.items()}
    assert paths["R13"] == {("whole", False, False, 0), ("word", False, False, 3)}
    assert paths["R15"] == {("whole", True, False, 0), ("whole", True, True, 0), ("word", True, False, 1), ("word", True, True, 1)}
    assert (1, 48, 28, 1) in VC.sad_workgroups(79, 127, 15, 15)                                   # the ragged bottom tile
    assert {(2, 48, 28, 1), (2, 48, 3, 2)} <= VC.sad_workgroups(80, 78, 15, 15)                   # a second tile row of height 2
    assert VC.sad_workgroups(80, 128, 16, 16) == {(48, 48, 28, 1), (48, 48, 5, 5)}
    assert VC.sad_workgroups(112, 113, 32, 32) == {(48, 48, 15, 1), (48, 48, 5, 3), (48, 1, 15, 1), (48, 1, 5, 3)}


@pytest.mark.parametrize("name", list(PATHS))
def test_path_cases_recover_their_shifts_in_every_chunk(name):
    frames, R, f, bgr = PATHS[name]
    true = VC.true_shifts(VC.path_offsets(name))
    assert frames.ndim == 3 and f == 1 and len(frames) >= 4 and np.array_equal(true, np.asarray(VC.PATH_SHAPES[name][3]))
    shifts, cost, surf = VO.frame_shifts(frames, R, f, bgr)
    assert np.array_equal(shifts, true) and not cost[:, 0].any() and (surf > 0).sum() == surf.size - len(true)
    D, _, CH = VC.sad_split(R)
    rows, cols = set((true[:, 0] + R).tolist()), set((true[:, 1] + R).tolist())
    assert {0, D - 1} <= cols                                                   # sx = -R and +R
    if CH < D:
        last = (D - 1) // CH * CH                                               # the first y-index of the short last chunk
        assert D % CH and any(i < CH for i in rows) and any(i >= last for i in rows) and {CH - 1, CH} <= rows


def test_carry_case_is_past_32_bits_and_past_one_grid_pass():
    H, W, R = VC.CARRY
    assert VC.CARRY_COST == 255 * (H - 2 * R) * (W - 2 * R) and 2**32 < VC.CARRY_COST < 2**33
    assert 2 * H * ((W + 3) // 4) > 4 * 256 * 32 * 256                          # words of the planes against frame_plane_kernel's largest grid


@pytest.mark.parametrize("period", list(VC.TIE_SHIFTS))
def test_ties_are_decided_by_each_key_in_turn(period):
    frames, R = VC.tie_frames(period), VC.TIE_RADIUS
    assert frames.shape == (2, 50, 58) and len(set(frames[0, :period[0], :period[1]].ravel().tolist())) == period[0] * period[1]
    shifts, cost, surf = VO.frame_shifts(frames, R, 1)
    assert shifts.tolist() == [list(VC.TIE_SHIFTS[period])] and not cost[:, 0].any()
    zeros = int((surf == 0).sum())
    assert surf.size == 361 > 256 and 60 <= zeros <= 100
    sy, sx = np.nonzero(surf[0] == 0)
    assert all((y - R - 1) % period[0] == 0 and (x - R - 1) % period[1] == 0 for y, x in zip(sy, sx))
    first = VO.frame_shifts(frames, R, 1, variant="first")[0]
    assert first.tolist() != shifts.tolist() and first[0, 0] < 0 and first[0, 1] < 0


def test_the_tie_keys_that_decide():
    """(2,2): four shifts at the smallest distance, sy then sx decide; (2,3) and (3,2): two, sy or sx decides; (1,4), (4,1): one"""
    nearest = {}
    for period in VC.TIE_SHIFTS:
        surf = VO.frame_shifts(VC.tie_frames(period), VC.TIE_RADIUS, 1)[2][0]
        z = [(int(y) - 9, int(x) - 9) for y, x in zip(*np.nonzero(surf == 0))]
        d2 = min(y * y + x * x for y, x in z)
        nearest[period] = sorted(s for s in z if s[0] ** 2 + s[1] ** 2 == d2)
    assert nearest == {(2, 2): [(-1, -1), (-1, 1), (1, -1), (1, 1)], (2, 3): [(-1, 1), (1, 1)], (3, 2): [(1, -1), (1, 1)], (1, 4): [(0, 1)],
                       (4, 1): [(1, 0)]}
    # a pick with the first two keys right and the index order reversed: only these frames tell it from the definition
    last = {p: VO.frame_shifts(VC.tie_frames(p), VC.TIE_RADIUS, 1, variant="last")[0].tolist()[0] for p in VC.TIE_SHIFTS}
    assert last == {(2, 2): [1, 1], (2, 3): [1, 1], (3, 2): [1, 1], (1, 4): [0, 1], (4, 1): [1, 0]}
    assert differs("last", list(CASES)) == []


def test_low_amplitude_planes_sit_on_rounding_edges():
    cases = VC.low_amplitude_cases()
    assert len(cases) == 7 and sorted({c[2] for c in cases.values()}) == [2, 4, 8] and sum(c[3] for c in cases.values()) == 1
    for name, (frames, R, f, bgr) in cases.items():
        H, W = frames.shape[1:3]
        assert H % f == f - 1 and W % f == f - 1 and (W // f) % 4 and R == 2
        y = VO.luma(frames, bgr)
        c = VO.coarse(y, f)
        lo = int(y.min())
        assert sorted(np.unique(y).tolist()) == [lo, lo + 1] and sorted(np.unique(c).tolist()) == [lo, lo + 1] and lo in (0, 254), name
        s = y[:, :H // f * f, :W // f * f].astype(np.int64).reshape(len(y), H // f, f, W // f, f).sum(axis=(2, 4))
        for wrong in (s // (f * f), (s + f * f // 2 - 1) // (f * f), (s + f * f - 1) // (f * f)):      # floor, half minus one, ceiling
            assert (wrong != c).mean() > 0.05, name
        more = VO.coarse(np.pad(y, ((0, 0), (0, 1), (0, 1)), constant_values=lo)[:, 1:, 1:], f)
        assert not np.array_equal(more, c)                                      # another block phase, another plane
        assert VO.frame_shifts(frames, R, f, bgr)[2].min() > 0


def test_alternating_columns_give_zero_or_the_maximum():
    frames, R, f, _ = VC.alternating_columns()
    shifts, cost, surf = VO.frame_shifts(frames, R, f)
    n = (frames.shape[1] - 2 * R) * (frames.shape[2] - 2 * R)
    assert set(np.unique(surf).tolist()) == {0, 255 * n} and shifts.tolist() == [[0, 0], [0, -1]]
    assert (surf[0][:, R % 2::2] == 0).all() and (surf[1][:, R % 2::2] == 255 * n).all()


# ---- many objects ---------------------------------------------------------------------------------------------------------------------
def test_many_links_table_is_what_it_says():
    off, link, cls = VC.many_links()
    frame = np.repeat(np.arange(6), VC.MANY_COUNTS)
    has = link >= 0
    assert np.diff(off).tolist() == VC.MANY_COUNTS and (link[has] < off[frame[has]]).all() and len(set(link[has].tolist())) == has.sum()
    back = frame[has] - frame[link[has]]
    assert set(back.tolist()) == {1, 2} and 30 <= (back == 2).sum() <= 40 and not has[:700].any()
    assert 100 < has[off[3]:off[4]].sum() < 160 and link[off[4]] >= 0 and frame[link[off[4]]] == 2
    assert set(frame[has][back == 2].tolist()) == {2, 4} and set(frame[VC.many_links((2,))[1] >= 0].tolist()) == {2, 3, 5}


def test_only_the_many_object_table_tells_a_rank_that_restarts_every_256():
    off, link, cls = VC.many_links()
    good, bad = VO.track_ids(off, link, cls), VO.track_ids(off, link, cls, variant="rank256")
    assert not np.array_equal(good[0], bad[0]) and good[1] != bad[1]
    assert good[1] == int((link < 0).sum()) and sorted(set(good[0].tolist())) == list(range(good[1]))
    hoff, hlink = np.array([0, 2, 5, 7, 7, 8], np.int64), np.array([-1, -1, 1, -1, 0, 3, 2, -1], np.int64)      # the hand-written table above
    hcls = np.array([1, 2, 2, 1, 1, 1, 2, 2], np.int64)
    a, b = VO.track_ids(hoff, hlink, hcls), VO.track_ids(hoff, hlink, hcls, variant="rank256")
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    frames, cls_map, _, shifts = VC.track_scene()                               # nor does the track scene
    labels, soff, scls, _ = VO.label_frames(cls_map)
    slink = VO.link_objects(labels, soff, scls, shifts, 0.3)
    a, b = VO.track_ids(soff, slink, scls), VO.track_ids(soff, slink, scls, variant="rank256")
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]


def merge_calls(off, link, cls, cuts, **kw):
    """the oracle run call by call over frames cuts[k][0] .. cuts[k][1], carried like mgu_track_ids' header says"""
    tid, nxt, lengths, classes, status = np.zeros(0, np.int64), 0, {}, {}, 0
    for k, (lo, hi) in enumerate(cuts):
        o, l, c = VC.cut_links(off, link, cls, lo, hi)
        first = tid[len(tid) - int(o[1]):] if k else None
        r = VO.track_ids(o, l, c, first_ids=first, next_id=nxt, **kw)
        tid, nxt, status = np.concatenate([tid, r[0][int(o[1]) if k else 0:]]), r[1], status | r[4]
        for key, v in r[2].items():
            lengths[key] = lengths.get(key, 0) + v
        classes.update(r[3])
    return tid, nxt, lengths, classes, status


@pytest.mark.parametrize("older,cuts", [((2, 4), ((0, 2), (2, 4), (4, 5))), ((2,), ((0, 2), (2, 3), (3, 5)))])
def test_many_objects_in_three_calls_equal_one(older, cuts):
    off, link, cls = VC.many_links(older)
    one = VO.track_ids(off, link, cls)
    got = merge_calls(off, link, cls, cuts)
    assert np.array_equal(got[0], one[0]) and got[1:] == one[1:]
    if older == (2,):
        assert all(VC.MANY_COUNTS[lo] >= 256 for lo, _ in cuts[1:])             # every carried frame takes more than one round


def test_object_capacity_rule():
    off, link, cls = VC.many_links()
    N = int(off[-1])
    full = VO.track_ids(off, link, cls)
    same = VO.track_ids(off, link, cls, object_capacity=N)
    assert np.array_equal(same[0], full[0]) and same[1:] == full[1:]
    cap = int(off[3]) + 100                                                     # inside frame 3: frames 4 and 5 are left out whole
    cut = VO.track_ids(off, link, cls, object_capacity=cap)
    assert cut[4] == 2 and np.array_equal(cut[0][:cap], full[0][:cap]) and (cut[0][cap:] == -1).all()
    assert cut[1] == int((link[:cap] < 0).sum()) < full[1] and sum(cut[2].values()) == cap


def test_dense_scene_has_hundreds_of_objects_a_frame():
    frames, cls, shifts = VC.dense_scene()
    labels, off, cid = VO.label_batch(cls)
    assert frames.shape == (3, 96, 128, 3) and all(250 <= n <= 340 for n in np.diff(off)) and set(cid.tolist()) == {1, 2}
    got, cost, _ = VO.frame_shifts(frames, VC.DENSE_RADIUS, 1)
    assert np.array_equal(got, shifts) and not cost[:, 0].any()
    link = VO.link_objects(labels, off, cid, shifts, 0.3)
    assert (link[off[1]:] >= 0).sum() > 400
    small = VC.track_scene()[1]                                                 # label_batch is label_frames on the track scene
    a, b = VO.label_frames(small), VO.label_batch(small)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b))
