"""The video kernels (csrc/video.hip) on the GPU against the numpy oracle (tests/video_oracle.py) on the shared cases
(tests/video_cases.py).  Everything is compared exactly: the coarse cost surface word for word, shifts, costs, the aligned label
maps, visible areas, links, track ids, lengths and classes; VideoCounter fed in chunks against one call; the launch counts and
run-to-run equality; count_video once on a tiny UNet."""
import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
import video_cases as VC
import video_oracle as VO
from mgunet import _lib

pytestmark = pytest.mark.gpu

CASES = VC.registration_cases()
_WANT = {}


def want(name):
    if name not in _WANT:
        frames, R, f, bgr = CASES[name]
        _WANT[name] = VO.frame_shifts(frames, R, f, bgr)
    return _WANT[name]


def run(cuda, name, surface=True):
    frames, R, f, bgr = CASES[name]
    out = mgunet.frame_shifts(torch.from_numpy(frames).to(cuda), R, f, bgr, return_surface=surface)
    return [o.cpu().numpy() for o in out]


def test_tile_size(cuda):
    assert int(_lib.lib().mgu_frame_sad_tile()) == VC.TILE


@pytest.mark.parametrize("name", list(CASES))
def test_registration_is_bitwise_the_oracle(cuda, name):
    shifts, cost, surf = run(cuda, name)
    ws, wc, wsurf = want(name)
    assert shifts.dtype == np.int32 and cost.dtype == np.int64 and surf.dtype == np.int64
    assert np.array_equal(surf, wsurf), name
    assert np.array_equal(shifts, ws) and np.array_equal(cost, wc), (name, shifts.tolist(), ws.tolist())
    s2, c2 = run(cuda, name, surface=False)                  # the surface in the context's scratch
    assert np.array_equal(s2, ws) and np.array_equal(c2, wc)


def test_the_special_frames_give_what_the_definition_says(cuda):
    for name in ("uniform", "uniform f2"):
        shifts, cost, surf = run(cuda, name)
        assert not shifts.any() and not cost.any() and not surf.any()
    frames, R, _, _ = CASES["0 vs 255"]
    shifts, cost, surf = run(cuda, "0 vs 255")
    n = (frames.shape[1] - 2 * R) * (frames.shape[2] - 2 * R)
    assert n >= 128 * 128 and (surf == 255 * n).all() and not shifts.any() and cost.tolist() == [[255 * n, 255 * n]]
    assert run(cuda, "corner")[0].tolist() == [[-5, 5]] and run(cuda, "corner f2")[0].tolist() == [[10, -10]]
    assert run(cuda, "f8 smallest")[0].tolist() == [[8, -8]]


@pytest.mark.parametrize("name", list(VC.KNOWN))
def test_known_shifts_come_back_with_cost_zero(cuda, name):
    offsets, H, W, ch, R, f = VC.KNOWN[name]
    frames = VC.crops(100 + f, H, W, offsets, ch)
    shifts, cost = mgunet.frame_shifts(torch.from_numpy(frames).to(cuda), R, f)
    assert np.array_equal(shifts.cpu().numpy(), VC.true_shifts(offsets)) and not cost[:, 0].any()


def test_rgb_bgr_and_grey_inputs_agree(cuda):
    frames = CASES["40x56 f1 R3"][0]
    a = mgunet.frame_shifts(torch.from_numpy(frames).to(cuda), 3, 1, False, True)
    b = mgunet.frame_shifts(torch.from_numpy(frames[..., ::-1].copy()).to(cuda), 3, 1, True, True)
    g = mgunet.frame_shifts(torch.from_numpy(VO.luma(frames)).to(cuda), 3, 1, False, True)
    swapped = mgunet.frame_shifts(torch.from_numpy(frames).to(cuda), 3, 1, True, True)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, g)) and not torch.equal(a[2], swapped[2])
    view = torch.from_numpy(frames).to(cuda)[:, :, 3:51]     # a strided view is taken as it is
    assert torch.equal(mgunet.frame_shifts(view, 3, 1)[0], torch.from_numpy(VO.frame_shifts(frames[:, :, 3:51], 3, 1)[0]).to(cuda))


def test_illegal_arguments_are_refused_with_a_message(cuda):
    z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=cuda)  # noqa: E731
    for args, msg in [((z(1, 40, 40), 2, 1), "at least 2 frames"), ((z(2, 40, 40), 0, 1), "radius"), ((z(2, 90, 90), 33, 1), "radius"),
                      ((z(2, 40, 40), 2, 3), "factor"), ((z(2, 23, 40), 8, 1), "window under 8 x 8"), ((z(2, 47, 48), 2, 4), "window under 8 x 8")]:
        with pytest.raises(ValueError, match=msg):
            mgunet.frame_shifts(*args)
    mgunet.frame_shifts(z(2, 24, 40), 8, 1), mgunet.frame_shifts(z(2, 48, 51), 2, 4)      # the smallest legal sizes
    with pytest.raises(TypeError):
        mgunet.frame_shifts(z(2, 40, 40, 4), 2, 1)
    with pytest.raises(TypeError):
        mgunet.frame_shifts(torch.zeros((2, 40, 40), device=cuda), 2, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mgunet.frame_shifts(torch.zeros((2, 40, 40), dtype=torch.uint8), 2, 1)
    L, ctx = _lib.lib(), _lib.context(cuda)
    f = z(2, 40, 40)
    assert L.mgu_frame_shifts(ctx.handle, f.data_ptr(), 2, 40, 40, 1, 0, 2, 1, None, None, None, None) == _lib.MGU_ERR_INVALID
    assert b"null pointer" in L.mgu_last_error(ctx.handle)


def launches(cuda, fn):
    ctx = _lib.context(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        fn()
        torch.cuda.synchronize()
        stats = _lib.read_kernel_stats(ctx)
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return {k["name"]: k["launches"] for k in stats}


def test_launch_counts_do_not_depend_on_the_frames(cuda):
    one = {"video planes": 1, "video sad": 1, "video pick": 1}
    for name in ("40x56 f1 R3", "T5 bgr", "uniform", "grey"):                      # T = 3, 5, 3, 2 at factor 1
        assert launches(cuda, lambda: run(cuda, name)) == one, name
    for name in ("67x93 f2 R4", "f4 R2", "uniform f2"):                            # T = 2, 3, 2 at factor > 1
        assert launches(cuda, lambda: run(cuda, name, surface=False)) == {k: 2 for k in one}, name


def test_two_runs_are_bitwise_equal(cuda):
    for name in ("R32", "67x93 f2 R4"):
        a, b = run(cuda, name), run(cuda, name)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- tracks --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    frames, cls, disc, shifts = VC.track_scene()
    labels, offsets, class_id, area = VO.label_frames(cls)
    link = VO.link_objects(labels, offsets, class_id, shifts, 0.3)
    return {"frames": frames, "cls": cls, "disc": disc, "shifts": shifts, "labels": labels, "offsets": offsets, "class_id": class_id, "area": area,
            "link": link, "ids": VO.track_ids(offsets, link, class_id)}


def test_links_and_track_ids_equal_the_oracle(cuda, scene):
    table = mgunet.connected_components(torch.from_numpy(scene["cls"]).to(cuda))
    assert np.array_equal(table.labels.cpu().numpy(), scene["labels"]) and np.array_equal(table.offsets.cpu().numpy(), scene["offsets"])
    shifts, cost = mgunet.frame_shifts(torch.from_numpy(scene["frames"]).to(cuda), VC.TRACK_RADIUS, 1)
    assert np.array_equal(shifts.cpu().numpy(), scene["shifts"]) and not cost[:, 0].any()
    link, (prev, nxt, vp, vn) = mgunet.link_objects(table, shifts, 0.3, return_aligned=True)
    wprev, wnxt, wvp, wvn = VO.track_align(scene["labels"], scene["offsets"], scene["shifts"])
    assert np.array_equal(prev.cpu().numpy(), wprev) and np.array_equal(nxt.cpu().numpy(), wnxt)
    assert np.array_equal(vp.cpu().numpy(), wvp) and np.array_equal(vn.cpu().numpy(), wvn)
    assert np.array_equal(link.cpu().numpy(), scene["link"])
    tid, next_id, tlen, tcls, status = mgunet.track_ids(table.offsets, link, table.class_id)
    wtid, wn, wlen, wcls, _ = scene["ids"]
    assert np.array_equal(tid.cpu().numpy(), wtid) and int(next_id) == wn and int(status) == 0
    assert tlen[:wn].cpu().tolist() == [wlen[k] for k in range(wn)] and tcls[:wn].cpu().tolist() == [wcls[k] for k in range(wn)]
    assert not tlen[wn:].any()
    # every disc is one track: the half-visible one (disc 5, frame 2) and the one that enters as a single pixel (disc 6, frame 3) too
    frame = np.repeat(np.arange(6), np.diff(scene["offsets"]))
    disc = np.array([int(scene["disc"][t][scene["labels"][t] == k][0]) - 1 for t in range(6) for k in range(1, int(np.diff(scene["offsets"])[t]) + 1)])
    ids = tid.cpu().numpy()
    assert all(len(set(ids[disc == d].tolist())) == 1 for d in set(disc.tolist())) and len(set(ids.tolist())) == len(set(disc.tolist()))
    assert ((disc == 5) & (frame == 2)).sum() == 1 and ((disc == 6) & (frame == 3)).sum() == 1
    # the same again: bitwise
    link2 = mgunet.link_objects(table, shifts, 0.3)
    assert torch.equal(link, link2) and torch.equal(mgunet.track_ids(table.offsets, link2, table.class_id)[0], tid)
    assert launches(cuda, lambda: mgunet.track_ids(table.offsets, mgunet.link_objects(table, shifts), table.class_id)) == {"track align": 1, "track ids": 1}


def test_score_order_and_classes(cuda):
    cls = np.zeros((2, 8, 12), np.int64)
    cls[0, 2:6, 2:10] = 1
    cls[1, 2:6, 2:6], cls[1, 2:6, 7:10] = 1, 1
    z = torch.zeros((1, 2), dtype=torch.int32, device=cuda)
    table = mgunet.connected_components(torch.from_numpy(cls).to(cuda))
    assert mgunet.link_objects(table, z).cpu().tolist() == [-1, 0, -1]
    assert mgunet.link_objects(table, z, scores=torch.tensor([0, 0.2, 0.9], device=cuda)).cpu().tolist() == [-1, -1, 0]
    cls[1, 2:6, 2:6] = 2
    assert mgunet.link_objects(mgunet.connected_components(torch.from_numpy(cls).to(cuda)), z).cpu().tolist() == [-1, -1, 0]
    with pytest.raises(ValueError, match="shifts"):
        mgunet.link_objects(table, z.to(torch.int64))


def counter(cuda, **kw):
    return mgunet.VideoCounter(3, cuda, radius=VC.TRACK_RADIUS, factor=1, iou=0.3, **kw)


def test_video_counter_in_chunks_equals_one_call(cuda, scene):
    frames, cls = torch.from_numpy(scene["frames"]).to(cuda), torch.from_numpy(scene["cls"]).to(cuda)
    whole = counter(cuda)
    whole.update(frames, cls)
    a = whole.compute()
    parts = counter(cuda)
    for lo, hi in ((0, 2), (2, 5), (5, 6)):
        parts.update(frames[lo:hi], cls[lo:hi])
    b = parts.compute()
    wtid, wn, wlen, wcls, _ = scene["ids"]
    off = scene["offsets"]
    for r in (a, b):
        assert r["tracks"] == wn and r["frames"] == 6 and r["frame_count_sum"] == int(off[-1])
        assert np.array_equal(r["shifts"], scene["shifts"])
        assert len(r["track_ids"]) == 6 and all(np.array_equal(r["track_ids"][t], wtid[off[t]:off[t + 1]]) for t in range(6))
        assert r["track_lengths"].tolist() == [wlen[k] for k in range(wn)] and r["track_classes"].tolist() == [wcls[k] for k in range(wn)]
        assert r["count"] == sum(v >= 2 for v in wlen.values()) and r["count"] < r["tracks"] < r["frame_count_sum"]
        assert r["count_per_class"] == [sum(1 for k in wlen if wlen[k] >= 2 and wcls[k] == c) for c in range(3)]
        assert sum(r["tracks_per_class"]) == wn
    single = counter(cuda, min_length=1)
    for t in range(6):
        single.update(frames[t:t + 1], cls[t:t + 1])
    c = single.compute()
    assert c["count"] == wn and all(np.array_equal(c["track_ids"][t], wtid[off[t]:off[t + 1]]) for t in range(6))


def test_capacity_overflow_sets_the_status_and_writes_nothing_past_the_arrays(cuda, scene):
    off, link, cid = (torch.from_numpy(scene[k]).to(cuda) for k in ("offsets", "link", "class_id"))
    wtid, wn = scene["ids"][:2]
    tlen, tcls = torch.full((wn,), 77, dtype=torch.int32, device=cuda), torch.full((wn,), 77, dtype=torch.int64, device=cuda)
    tlen[:3], tcls[:3] = 0, -1
    tid, next_id, _, _, status = mgunet.track_ids(off, link, cid, tracks=(tlen[:3], tcls[:3]))
    assert int(status) == 1 and int(next_id) == wn and np.array_equal(tid.cpu().numpy(), wtid)
    assert (tlen[3:] == 77).all() and (tcls[3:] == 77).all() and tlen[:3].cpu().tolist() == [scene["ids"][2][k] for k in range(3)]
    assert int(mgunet.track_ids(off, link, cid, track_capacity=wn)[4]) == 0
    small = counter(cuda, max_tracks=3)
    small.update(torch.from_numpy(scene["frames"]).to(cuda), torch.from_numpy(scene["cls"]).to(cuda))
    with pytest.raises(RuntimeError, match="max_tracks"):
        small.compute()


def test_count_video_on_a_tiny_unet(cuda, scene):
    cfg = (3, 3, 8, 2)
    model = mgunet.UNet(*cfg)
    model.load_state_dict(O.make_unet_params(*cfg, seed=7))
    model = model.to(cuda)
    frames = torch.from_numpy(scene["frames"])
    r = mgunet.count_video(model, frames, chunk=4, radius=VC.TRACK_RADIUS, factor=1, min_area=4)
    assert r["frames"] == 6 and np.array_equal(r["shifts"], scene["shifts"]) and model.training
    assert 0 <= r["count"] <= r["tracks"] <= r["frame_count_sum"] and sum(len(x) for x in r["track_ids"]) == r["frame_count_sum"]
    vc = mgunet.VideoCounter(3, cuda, radius=VC.TRACK_RADIUS, factor=1, min_area=4)      # the same composition by hand
    model.eval()
    with torch.no_grad():
        for lo in (0, 4):
            u8 = frames[lo:lo + 4].to(cuda)
            vc.update(u8, model((u8.float() / 255.0).permute(0, 3, 1, 2).contiguous())[0])
    one = vc.compute()
    assert one["tracks"] == r["tracks"] and one["count"] == r["count"] and all(np.array_equal(x, y) for x, y in zip(one["track_ids"], r["track_ids"]))
