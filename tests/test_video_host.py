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
