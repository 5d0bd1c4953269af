"""The video kernels (csrc/video.hip) where tests/test_gpu_video.py does not reach: every work split of frame_sad_kernel (whole-row
and word path, with and without y-shift chunks, rows whole or sliced: tests/video_cases.py mirrors the split and the host suite holds
the case tables against it), costs above 2^32, ties that each key of the pick decides, planes on rounding edges; track_align on a
hand-written shift table, with every lane of a wave on another object, under a small capacity and past one pass of its grid;
track_ids over rounds of 256 objects, in carried calls and past both capacities; link_objects and VideoCounter on hundreds of
objects a frame.  Everything is an exact comparison with the numpy oracle (tests/video_oracle.py); a mismatch is reported with its
index and both values."""
import numpy as np
import pytest
import torch

import mgunet
import video_cases as VC
import video_oracle as VO
from mgunet import _lib
from mgunet.video import _ids

pytestmark = pytest.mark.gpu


def same(got, want, what):
    got, want = np.asarray(got.cpu() if torch.is_tensor(got) else got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} differ, the first at {at}: got {got[at]}, want {want[at]}")


def registers_like_the_oracle(cuda, name, case, want=None):
    """surface, shifts and costs of a (frames, radius, factor, bgr) case against the oracle, with the surface returned and in scratch"""
    frames, R, f, bgr = case
    ws, wc, wsurf = want or VO.frame_shifts(frames, R, f, bgr)
    dev = torch.from_numpy(frames).to(cuda)
    shifts, cost, surf = mgunet.frame_shifts(dev, R, f, bgr, return_surface=True)
    same(surf, wsurf, f"{name}: surface [pair, sy + R, sx + R]")
    same(shifts, ws, f"{name}: shifts")
    same(cost, wc, f"{name}: cost")
    s2, c2 = mgunet.frame_shifts(dev, R, f, bgr)                       # the surface in the context's scratch
    same(s2, ws, f"{name}: shifts, surface in scratch")
    same(c2, wc, f"{name}: cost, surface in scratch")
    return ws, wc, wsurf


# ---- 1. every work split of frame_sad_kernel ------------------------------------------------------------------------------------------
PATHS = VC.path_cases()


@pytest.mark.parametrize("name", list(PATHS))
def test_every_work_split_gives_the_oracles_surface(cuda, name):
    ws, wc, _ = registers_like_the_oracle(cuda, name, PATHS[name])
    assert np.array_equal(ws, VC.true_shifts(VC.path_offsets(name))) and not wc[:, 0].any()


# ---- 2. contents ----------------------------------------------------------------------------------------------------------------------
def test_costs_above_32_bits_carry_into_the_upper_word(cuda):
    H, W, R = VC.CARRY
    frames = torch.zeros((2, H, W), dtype=torch.uint8, device=cuda)   # made on the device: 34 MB that never cross the bus
    frames[1] = 255
    shifts, cost, surf = mgunet.frame_shifts(frames, R, 1, return_surface=True)
    same(surf, np.full((1, 3, 3), VC.CARRY_COST, np.int64), "carry: surface")
    assert shifts.cpu().tolist() == [[0, 0]] and cost.cpu().tolist() == [[VC.CARRY_COST, VC.CARRY_COST]]
    s2, c2 = mgunet.frame_shifts(frames, R, 1)
    assert s2.cpu().tolist() == [[0, 0]] and c2.cpu().tolist() == [[VC.CARRY_COST, VC.CARRY_COST]]


@pytest.mark.parametrize("period", list(VC.TIE_SHIFTS))
def test_ties_go_to_the_nearest_then_the_smaller_sy_then_the_smaller_sx(cuda, period):
    ws, wc, wsurf = registers_like_the_oracle(cuda, f"ties {period}", (VC.tie_frames(period), VC.TIE_RADIUS, 1, False))
    assert ws.tolist() == [list(VC.TIE_SHIFTS[period])] and not wc[:, 0].any() and 60 <= (wsurf == 0).sum() <= 100    # the literal shifts


LOW = VC.low_amplitude_cases()


@pytest.mark.parametrize("name", list(LOW))
def test_low_amplitude_planes(cuda, name):
    registers_like_the_oracle(cuda, name, LOW[name])


def test_alternating_columns(cuda):
    _, _, wsurf = registers_like_the_oracle(cuda, "alternating columns", VC.alternating_columns())
    assert len(np.unique(wsurf)) == 2


# ---- 3. track_align alone -------------------------------------------------------------------------------------------------------------
def table_of(cuda, cls, connectivity=2):
    """connected_components of a class map, held against the object tests' oracle first -> (table, labels, offsets, class_id)"""
    labels, offsets, cid = VO.label_batch(cls, connectivity)
    table = mgunet.connected_components(torch.from_numpy(cls).to(cuda), connectivity)
    same(table.labels, labels, "labels")
    same(table.offsets, offsets, "offsets")
    same(table.class_id, cid, "class_id")
    return table, labels, offsets, cid


def aligns_like_the_oracle(cuda, what, table, labels, offsets, shifts):
    shifts = np.asarray(shifts, np.int32)
    _, got = mgunet.link_objects(table, torch.from_numpy(shifts).to(cuda), 0.3, return_aligned=True)
    want = VO.track_align(labels, offsets, shifts)
    for g, w, k in zip(got, want, ("prev_aligned", "next_cropped", "vis_prev", "vis_next")):
        same(g, w, f"{what}: {k}")
    return want


def test_track_align_on_a_hand_written_shift_table(cuda):
    H, W = VC.ALIGN_HW
    table, labels, offsets, _ = table_of(cuda, VC.align_maps())
    assert len(VC.ALIGN_SHIFTS) == 8 and np.diff(offsets).min() >= 5
    for lo in (0, 1):                                                  # eight shifts over the seven pairs of T = 8, twice
        sh = VC.ALIGN_SHIFTS[lo:lo + 7]
        prev, nxt, vp, vn = aligns_like_the_oracle(cuda, f"shifts {lo}..{lo + 6}", table, labels, offsets, sh)
        for b, (sy, sx) in enumerate(sh):
            kept = max(0, H - abs(sy)) * max(0, W - abs(sx))           # pixels of the common rectangle
            assert (prev[b] > 0).sum() <= kept and (nxt[b] > 0).sum() <= kept
            assert bool(prev[b].any()) == bool(nxt[b].any()) == (kept > 0), (lo, b)      # a one-line rectangle holds objects, an empty one none


def test_track_align_with_every_lane_on_another_object(cuda):
    cls, shifts = VC.checkerboard_maps()
    table, labels, offsets, _ = table_of(cuda, cls, connectivity=1)
    assert np.diff(offsets).tolist() == [247, 1, 247] and 247 % 64
    prev, nxt, vp, vn = aligns_like_the_oracle(cuda, "checkerboard", table, labels, offsets, shifts)
    assert set(vp[:247].tolist()) == {0, 1} and vp[247] == 13 * 16 and vn[247] == 12 * 17 and set(vn[248:].tolist()) == {0, 1}


def raw_align(cuda, labels, offsets, cap, shifts, guard):
    T, H, W = labels.shape
    N = int(offsets[-1])
    lab, off, sh = (torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (labels, offsets, np.asarray(shifts, np.int32)))
    prev, nxt = (torch.full((T - 1, H, W), -5, dtype=torch.int32, device=cuda) for _ in range(2))
    vp, vn = (torch.full((N,), guard, dtype=torch.int64, device=cuda) for _ in range(2))
    _lib.call("mgu_track_align", cuda, lab, off, int(cap), sh, T, H, W, prev, nxt, vp, vn)
    return prev, nxt, vp, vn


def test_track_align_counts_nothing_past_its_capacity(cuda):
    H, W = VC.ALIGN_HW
    labels, offsets, _ = VO.label_batch(VC.align_maps())
    shifts = [(0, 0), (3, -4), (-3, 4), (1, 1), (0, -2), (2, 0), (0, 0)]
    wprev, wnxt, wvp, wvn = VO.track_align(labels, offsets, shifts)
    N = int(offsets[-1])
    assert wvn[N - 5:].all() and wvp[int(offsets[4]) + 2:].sum() > 100                    # the objects left out are visible
    for cap in (N - 5, int(offsets[4]) + 2):
        prev, nxt, vp, vn = raw_align(cuda, labels, offsets, cap, shifts, guard=-77)
        same(prev, wprev, f"capacity {cap}: prev_aligned")
        same(nxt, wnxt, f"capacity {cap}: next_cropped")
        same(vp[:cap], wvp[:cap], f"capacity {cap}: vis_prev")
        same(vn[:cap], wvn[:cap], f"capacity {cap}: vis_next")
        assert (vp[cap:] == -77).all() and (vn[cap:] == -77).all()


def test_track_align_past_one_pass_of_its_grid(cuda):
    T, H, W = 10, 512, 512
    assert (T - 1) * H * W > 2**21
    table, labels, offsets, _ = table_of(cuda, VC.blob_maps(61, T, H, W, 40, size=(4, 20)))
    assert 250 <= offsets[-1] <= 400
    shifts = np.random.default_rng(62).integers(-20, 21, (T - 1, 2)).astype(np.int32)
    aligns_like_the_oracle(cuda, "10 x 512 x 512", table, labels, offsets, shifts)


# ---- 4. track_ids over rounds of 256 objects --------------------------------------------------------------------------------------------
def on(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def same_tracks(what, got, want, capacity=None):
    tid, next_id, tlen, tcls, status = got
    wtid, wn, wlen, wcls, wst = want
    same(tid, wtid, f"{what}: track_id")
    assert int(next_id) == wn and int(status) == wst, (what, int(next_id), wn, int(status), wst)
    n = tlen.numel() if capacity is None else capacity
    same(tlen[:n], [wlen.get(k, 0) for k in range(n)], f"{what}: track_len")
    same(tcls[:n], [wcls.get(k, -1) for k in range(n)], f"{what}: track_class")


@pytest.mark.parametrize("older", [(2, 4), (2,)])
def test_track_ids_of_many_objects(cuda, older):
    off, link, cls = VC.many_links(older)
    want = VO.track_ids(off, link, cls)
    assert want[1] > 1024 and want[4] == 0
    a = mgunet.track_ids(*on(cuda, off, link, cls))
    same_tracks("one call", a, want)
    b = mgunet.track_ids(*on(cuda, off, link, cls))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("older,cuts", [((2, 4), ((0, 2), (2, 4), (4, 5))), ((2,), ((0, 2), (2, 3), (3, 5)))])
def test_track_ids_in_three_carried_calls_equal_one(cuda, older, cuts):
    off, link, cls = VC.many_links(older)
    want = VO.track_ids(off, link, cls)
    N = int(off[-1])
    next_id = torch.zeros(1, dtype=torch.int64, device=cuda)
    tracks = (torch.zeros(N, dtype=torch.int32, device=cuda), torch.full((N,), -1, dtype=torch.int64, device=cuda))
    ids, status, first = [], 0, None
    for k, (lo, hi) in enumerate(cuts):
        o, l, c = VC.cut_links(off, link, cls, lo, hi)
        tid, next_id, _, _, st = mgunet.track_ids(*on(cuda, o, l, c), first_ids=first, next_id=next_id, tracks=tracks)
        n_first, n_last = int(o[1]), int(o[-1] - o[-2])
        if k:
            assert torch.equal(tid[:n_first], first)                   # the carried ids are kept
        ids.append(tid[n_first if k else 0:])
        first = tid[tid.numel() - n_last:].clone()
        status |= int(st)
    same_tracks(f"cuts {cuts}", (torch.cat(ids), next_id, *tracks, status), want)


def test_track_capacity_overflow_in_a_later_round(cuda):
    off, link, cls = VC.many_links()
    cap = 600                                                          # id 600 is handed out in frame 0's third round of 256
    want = VO.track_ids(off, link, cls, capacity=cap)
    full = VO.track_ids(off, link, cls)
    assert want[4] == 1 and want[1] == full[1] > cap and np.array_equal(want[0], full[0])
    tlen, tcls = torch.full((cap + 64,), 77, dtype=torch.int32, device=cuda), torch.full((cap + 64,), 77, dtype=torch.int64, device=cuda)
    tlen[:cap], tcls[:cap] = 0, -1
    got = mgunet.track_ids(*on(cuda, off, link, cls), tracks=(tlen[:cap], tcls[:cap]))
    same_tracks("track_capacity 600", got, want)
    assert (tlen[cap:] == 77).all() and (tcls[cap:] == 77).all()
    assert int(mgunet.track_ids(*on(cuda, off, link, cls), track_capacity=full[1])[4]) == 0
    assert int(mgunet.track_ids(*on(cuda, off, link, cls), track_capacity=full[1] - 1)[4]) == 1


def raw_ids(cuda, off, link, cls, cap, tcap, first=None, next_id=0):
    N = int(off[-1])
    o, l, c = on(cuda, off, link, cls)
    nid = torch.tensor([next_id], dtype=torch.int64, device=cuda)
    tid = torch.full((max(N, 1),), -7, dtype=torch.int64, device=cuda)
    tlen, tcls = torch.zeros(tcap, dtype=torch.int32, device=cuda), torch.full((tcap,), -1, dtype=torch.int64, device=cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    _ids(o, len(off) - 1, cap, l, c, None if first is None else on(cuda, first)[0], nid, tid, tlen, tcls, status)
    return tid, nid, tlen, tcls, status


def test_object_capacity_below_the_object_count(cuda):
    off, link, cls = VC.many_links()
    N = int(off[-1])
    for cap in (int(off[3]) + 100, int(off[5]) + 300, int(off[1]) - 1, 0):       # inside frames 3, 5 and 0; nothing at all
        want = VO.track_ids(off, link, cls, object_capacity=cap)
        tid, nid, tlen, tcls, status = raw_ids(cuda, off, link, cls, cap, N)
        assert want[4] == 2 and (tid[cap:] == -7).all(), cap                     # nothing is written past capacity
        same_tracks(f"capacity {cap}", (tid[:cap], nid, tlen, tcls, status), (want[0][:cap],) + want[1:])
    want = VO.track_ids(off, link, cls, capacity=600, object_capacity=int(off[3]) + 100)
    got = raw_ids(cuda, off, link, cls, int(off[3]) + 100, 600)
    assert want[4] == 3 and int(got[4]) == 3
    same(got[0][:int(off[3]) + 100], want[0][:int(off[3]) + 100], "both capacities: track_id")


def test_track_ids_of_one_frame(cuda):
    off, link, cls = np.array([0, 300], np.int64), np.full(300, -1, np.int64), np.arange(300, dtype=np.int64) % 2 + 1
    got = mgunet.track_ids(*on(cuda, off, link, cls))
    same_tracks("T = 1", got, VO.track_ids(off, link, cls))
    assert got[0].cpu().tolist() == list(range(300)) and int(got[1]) == 300
    first = np.arange(300, dtype=np.int64)[::-1] * 3
    want = VO.track_ids(off, link, cls, first_ids=first, next_id=900)
    got = raw_ids(cuda, off, link, cls, 300, 16, first=first, next_id=900)       # a carried frame alone: ids kept, nothing counted
    same_tracks("T = 1 carried", got, want)
    assert want[1] == 900 and not want[2] and not got[2].any()
    empty = raw_ids(cuda, np.array([0, 0], np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64), 0, 4, next_id=5)
    assert int(empty[1]) == 5 and int(empty[4]) == 0 and int(empty[0][0]) == -7


# ---- 5. link_objects and VideoCounter on hundreds of objects a frame ------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense():
    frames, cls, shifts = VC.dense_scene()
    labels, offsets, cid = VO.label_batch(cls)
    link = VO.link_objects(labels, offsets, cid, shifts, 0.3)
    return {"frames": frames, "cls": cls, "shifts": shifts, "labels": labels, "offsets": offsets, "class_id": cid, "link": link,
            "ids": VO.track_ids(offsets, link, cid)}


def test_dense_links_equal_the_oracle(cuda, dense):
    table, labels, offsets, cid = table_of(cuda, dense["cls"])
    assert all(250 <= n <= 340 for n in np.diff(offsets))
    shifts = torch.from_numpy(dense["shifts"]).to(cuda)
    aligns_like_the_oracle(cuda, "dense", table, labels, offsets, dense["shifts"])
    link = mgunet.link_objects(table, shifts, 0.3)
    same(link, dense["link"], "dense: link")
    N = int(offsets[-1])
    scores = (np.random.default_rng(63).integers(0, 4, N) / 4).astype(np.float32)          # four values: exact ties everywhere
    by_score = mgunet.link_objects(table, shifts, 0.3, scores=torch.from_numpy(scores).to(cuda))
    wscore = VO.link_objects(labels, offsets, cid, dense["shifts"], 0.3, scores=scores)
    same(by_score, wscore, "dense: link by score")
    assert torch.equal(mgunet.link_objects(table, shifts, 0.3), link)
    # registered two pixels off and with a low threshold the objects compete for their neighbours: the visiting order decides
    off2 = dense["shifts"] + np.array([2, -2], np.int32)
    wlist, wscore = VO.link_objects(labels, offsets, cid, off2, 0.05), VO.link_objects(labels, offsets, cid, off2, 0.05, scores=scores)
    assert (wlist != wscore).sum() >= 10 and (wlist >= 0).sum() > 200
    args = (table, torch.from_numpy(off2).to(cuda), 0.05)
    same(mgunet.link_objects(*args), wlist, "dense, 2 px off: link")
    by_score = mgunet.link_objects(*args, scores=torch.from_numpy(scores).to(cuda))
    same(by_score, wscore, "dense, 2 px off: link by score")
    assert torch.equal(mgunet.link_objects(*args, scores=torch.from_numpy(scores).to(cuda)), by_score)


def test_equal_overlaps_go_to_the_smaller_index(cuda):
    cls = np.zeros((2, 24, 28), np.int64)
    cls[0, 2:6, 2:6], cls[0, 2:6, 8:12] = 1, 1                        # objects 0, 1: side by side
    cls[0, 10:14, 20:24], cls[0, 16:20, 20:24] = 1, 1                 # objects 2, 3: one above the other
    cls[1, 2:6, 4:10] = 1                                             # object 4 covers 8 pixels of each of 0 and 1
    cls[1, 12:18, 20:24] = 1                                          # object 5 covers 8 pixels of each of 2 and 3
    table, labels, offsets, cid = table_of(cuda, cls)
    z = np.zeros((1, 2), np.int32)
    want = VO.link_objects(labels, offsets, cid, z, 0.2)
    assert want.tolist() == [-1, -1, -1, -1, 0, 2]
    same(mgunet.link_objects(table, torch.from_numpy(z).to(cuda), 0.2), want, "IoU tie")


def test_video_counter_on_the_dense_scene_whole_and_in_chunks(cuda, dense):
    frames, cls = torch.from_numpy(dense["frames"]).to(cuda), torch.from_numpy(dense["cls"]).to(cuda)
    make = lambda: mgunet.VideoCounter(3, cuda, radius=VC.DENSE_RADIUS, factor=1, iou=0.3)  # noqa: E731
    whole = make()
    whole.update(frames, cls)
    a = whole.compute()
    parts = make()
    for lo, hi in ((0, 1), (1, 3)):
        parts.update(frames[lo:hi], cls[lo:hi])
    b = parts.compute()
    wtid, wn, wlen, wcls, _ = dense["ids"]
    off = dense["offsets"]
    for what, r in (("whole", a), ("chunks", b)):
        assert r["tracks"] == wn and r["frames"] == 3 and r["frame_count_sum"] == int(off[-1]), what
        same(r["shifts"], dense["shifts"], f"{what}: shifts")
        for t in range(3):
            same(r["track_ids"][t], wtid[off[t]:off[t + 1]], f"{what}: ids of frame {t}")
        same(r["track_lengths"], [wlen[k] for k in range(wn)], f"{what}: track_lengths")
        same(r["track_classes"], [wcls[k] for k in range(wn)], f"{what}: track_classes")
        assert r["count"] == sum(v >= 2 for v in wlen.values()) and 256 < r["count"] < r["tracks"] < r["frame_count_sum"]
        assert r["count_per_class"] == [sum(1 for k in wlen if wlen[k] >= 2 and wcls[k] == c) for c in range(3)]
        assert r["tracks_per_class"] == [sum(1 for k in wcls if wcls[k] == c) for c in range(3)]
