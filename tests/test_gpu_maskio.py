"""The mask input / output kernels (csrc/maskio.hip) on the GPU, every entry point bitwise equal to tests/maskio_oracle.py on the
cases of tests/maskio_cases.py and run twice: runs, runs back to labels, outlines, polygon fill; the round trips; capacities one short
of need; the launch count; refused arguments; COCO dictionaries in and out; annotations as an ObjectTable under object_overlaps and
match_masks."""
import functools

import numpy as np
import pytest
import torch

import maskio_cases as MC
import maskio_oracle as MO
import mgunet
from mgunet import _lib, maskio

pytestmark = pytest.mark.gpu

CASES = MC.label_cases()
FILLS = MC.fill_cases()
FAST_FILL = [n for n, c in CASES.items() if c["labels"].size <= 3000]     # the oracle's fill is per pixel and edge


def clean(case):
    lab = case["labels"].copy()
    lab[(lab < 1) | (lab > np.diff(case["offsets"])[:, None, None])] = 0
    return lab


@functools.lru_cache(maxsize=None)
def want_runs(name):
    return MO.encode(CASES[name]["labels"], CASES[name]["offsets"])


@functools.lru_cache(maxsize=None)
def want_outlines(name, c):
    return MO.outlines(CASES[name]["labels"], CASES[name]["offsets"], c)


def on_device(cuda, case):
    return torch.from_numpy(case["labels"]).to(cuda), torch.from_numpy(case["offsets"]).to(cuda)


def same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in a.__dataclass_fields__ if isinstance(getattr(a, f), torch.Tensor))


def check_runs(t, want):
    ptr, start, length = want
    R = len(start)
    assert int(t.status.item()) == 0
    assert np.array_equal(t.run_ptr.cpu().numpy(), ptr)
    assert np.array_equal(t.run_start[:R].cpu().numpy(), start) and np.array_equal(t.run_length[:R].cpu().numpy(), length)


def check_outlines(t, want):
    lp, vp, v, a2 = want
    L, V = len(a2), len(v)
    assert int(t.status.item()) == 0
    assert np.array_equal(t.loop_ptr.cpu().numpy(), lp) and np.array_equal(t.vertex_ptr[:L + 1].cpu().numpy(), vp)
    assert np.array_equal(t.vertices[:V].cpu().numpy(), v) and np.array_equal(t.loop_area2[:L].cpu().numpy(), a2)
    assert bool((t.vertex_ptr[L:] == V).all())


@pytest.mark.parametrize("name", list(CASES))
def test_runs_and_back_against_the_oracle(cuda, name):
    case = CASES[name]
    lab, off = on_device(cuda, case)
    t, again = mgunet.encode_masks((lab, off)), mgunet.encode_masks((lab, off))
    check_runs(t, want_runs(name))
    assert same(t, again)
    area = np.array([int(m.sum()) for _, _, m in MO.object_masks(case["labels"], case["offsets"])], np.int64)
    assert np.array_equal(t.areas().cpu().numpy(), area)
    back, counts, offsets, status = mgunet.labels_from_runs(t, return_status=True)
    assert int(status.item()) == 0 and np.array_equal(back.cpu().numpy(), clean(case))
    assert torch.equal(back, mgunet.labels_from_runs(t)[0]) and torch.equal(counts, off[1:] - off[:-1])


@pytest.mark.parametrize("name", list(CASES))
def test_outlines_and_back_against_the_oracle(cuda, name):
    case = CASES[name]
    lab, off = on_device(cuda, case)
    for c in ((1, 2) if name in FAST_FILL else (case["connectivity"],)):
        t, again = mgunet.object_outlines((lab, off), c), mgunet.object_outlines((lab, off), c)
        want = want_outlines(name, c)
        check_outlines(t, want)
        assert same(t, again)
        lp, a2 = want[0], want[3]
        area = np.array([int(m.sum()) for _, _, m in MO.object_masks(case["labels"], case["offsets"])], np.int64)
        assert all(int(a2[lp[i]:lp[i + 1]].sum()) == 2 * area[i] for i in range(len(area)))        # property (a)
        back, _, _, status = mgunet.rasterize_polygons(t, return_status=True)                       # property (d)
        assert int(status.item()) == 0 and np.array_equal(back.cpu().numpy(), clean(case)), c


def test_default_capacities_are_reached_exactly(cuda):
    lab, off = on_device(cuda, CASES["every_pixel_65x63"])
    n = 65 * 63
    r, o = mgunet.encode_masks((lab, off)).check(), mgunet.object_outlines((lab, off), 1).check()
    assert int(r.run_ptr[-1]) == n == r.run_capacity
    assert int(o.loop_ptr[-1]) == n == o.loop_capacity and int(o.vertex_ptr[-1]) == 4 * n == o.vertex_capacity
    full = MC.batch([MC.full_frame(7, 5)], 2)
    r, o = mgunet.encode_masks(on_device(cuda, full)), mgunet.object_outlines(on_device(cuda, full))
    assert (r.run_start[0].item(), r.run_length[0].item(), r.run_ptr.tolist()) == (0, 35, [0, 1])
    assert o.vertices[:4].tolist() == [[0, 0], [5, 0], [5, 7], [0, 7]] and o.vertex_ptr[:2].tolist() == [0, 4] and o.loop_area2[0].item() == 70


def raw_fill(cuda, table, cap=None):
    lp, vp, v, off, B, H, W, f = table
    cap = maskio._crossings(v, vp, H, f) if cap is None else cap
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (lp, vp, v, off)]
    return maskio._fill(cuda, *dev, B, H, W, f, cap, True)


@pytest.mark.parametrize("name", list(FILLS))
def test_fill_against_the_oracle(cuda, name):
    table = MC.fill_table(FILLS[name])
    want = MO.fill(*table)
    got, again = raw_fill(cuda, table), raw_fill(cuda, table)
    assert int(got[3].item()) == 0 and np.array_equal(got[0].cpu().numpy(), want)
    assert torch.equal(got[0], again[0])
    c = FILLS[name]
    listed = [[(0, loops) for loops in per] for per in c["polygons"]]
    lab, counts, offsets = mgunet.rasterize_polygons(listed, c["size"], c["frac_bits"], device=cuda)
    assert torch.equal(lab, got[0]) and offsets.tolist() == table[3].tolist()
    roomy = raw_fill(cuda, table, cap=5000)
    assert torch.equal(roomy[0], got[0])


def test_overlapping_and_invalid_runs(cuda):
    H, W, off = 4, 5, np.array([0, 3, 3, 4], np.int64)
    ptr = np.array([0, 2, 4, 6, 8], np.int64)
    start = np.array([0, 9, 2, 9, 18, 1, 0, 15], np.int32)
    length = np.array([6, 4, 5, 2, 2, 0, 20, 6], np.int32)            # (1, 0): length < 1; (15, 6): past H*W; row 2 ends at H*W exactly
    want, wst = MO.decode(ptr, start, length, off, 3, H, W)
    t = maskio.RunTable(*(torch.from_numpy(a).to(cuda) for a in (ptr, start, length)), torch.zeros(1, dtype=torch.int32, device=cuda),
                        torch.from_numpy(off).to(cuda), (3, H, W))
    lab, _, _, status = mgunet.labels_from_runs(t, return_status=True)
    assert wst == 1 and int(status.item()) == 1 and np.array_equal(lab.cpu().numpy(), want)
    assert want[0].max() == 3 and (want[2] == 1).all() and not want[1].any()
    neg = maskio.RunTable(t.run_ptr, torch.tensor([-1, 9, 2, 9, 18, 1, 0, 15], dtype=torch.int32, device=cuda), t.run_length, t.status, t.offsets, t.size)
    assert int(mgunet.labels_from_runs(neg, return_status=True)[3].item()) == 1


def test_capacities_one_short_keep_the_complete_rows(cuda):
    name = "scene_7x5_b3"
    case = CASES[name]
    lab, off = on_device(cuda, case)
    ptr, start, length = want_runs(name)
    R = len(start)
    t = mgunet.encode_masks((lab, off), run_capacity=R - 1)
    assert int(t.status.item()) == 1 and np.array_equal(t.run_ptr.cpu().numpy(), ptr)
    assert np.array_equal(t.run_start.cpu().numpy(), start[:R - 1]) and np.array_equal(t.run_length.cpu().numpy(), length[:R - 1])
    with pytest.raises(RuntimeError, match="run_capacity"):
        t.check()
    assert int(mgunet.labels_from_runs(t, return_status=True)[3].item()) == 4
    lp, vp, v, a2 = want_outlines(name, 2)
    L, V = len(a2), len(v)
    t = mgunet.object_outlines((lab, off), 2, loop_capacity=L - 1)
    assert int(t.status.item()) == 1 and np.array_equal(t.loop_ptr.cpu().numpy(), lp)
    assert np.array_equal(t.vertex_ptr.cpu().numpy(), vp[:L]) and np.array_equal(t.loop_area2.cpu().numpy(), a2[:L - 1])
    assert np.array_equal(t.vertices[:vp[L - 1]].cpu().numpy(), v[:vp[L - 1]])
    with pytest.raises(RuntimeError, match="loop_capacity"):
        t.check()
    t = mgunet.object_outlines((lab, off), 2, vertex_capacity=V - 1)
    assert int(t.status.item()) == 2 and np.array_equal(t.vertices.cpu().numpy(), v[:V - 1])
    assert np.array_equal(t.vertex_ptr[:L + 1].cpu().numpy(), vp) and np.array_equal(t.loop_area2[:L].cpu().numpy(), a2)
    with pytest.raises(RuntimeError, match="vertex_capacity"):
        t.check()
    table = MC.fill_table(FILLS["overlap"])
    need = maskio._crossings(table[2], table[1], table[5], table[7])
    got = raw_fill(cuda, table, cap=need - 1)
    want = MO.fill(*table)
    last = (want[2] == 2)                                               # the object whose edges come last loses a crossing
    assert int(got[3].item()) == 1 and np.array_equal(got[0].cpu().numpy()[:2], want[:2])
    assert np.array_equal(got[0].cpu().numpy()[2][~last], want[2][~last])


def count_launches(cuda, fn):
    ctx = _lib.context(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        fn()
        torch.cuda.synchronize(cuda)
        stats = _lib.read_kernel_stats(ctx)
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return sum(k["launches"] for k in stats)


def test_launch_count_depends_on_the_sizes_alone(cuda):
    """the empty image, the scene and the checkerboard at one (H, W) and one object capacity"""
    H, W = 65, 63
    maps = {"empty": MC.empty(H, W), "scene": MC.random_map(H, W, 0.5, 2, 1), "checkerboard": MC.checkerboard(H, W, 1), "full": MC.full_frame(H, W)}
    cap, n = H * W, H * W
    got = {}
    for name, m in maps.items():
        for B in (1, 2):
            lab, off = on_device(cuda, MC.batch([m] * B, 2))
            mk = lambda k, dt: torch.zeros(k, dtype=dt, device=cuda)  # noqa: E731
            st = mk(1, torch.int32)
            rp, rs, rl = mk(cap + 1, torch.int64), mk(B * n, torch.int32), mk(B * n, torch.int32)
            lp, vp, vs, a2 = mk(cap + 1, torch.int64), mk(B * n + 1, torch.int64), mk(8 * B * n, torch.int32), mk(B * n, torch.int64)
            out = mk(B * n, torch.int32)
            calls = {"runs": lambda: _lib.call("mgu_mask_runs", cuda, lab, off, cap, B, H, W, B * n, rp, rs, rl, st),
                     "paint": lambda: _lib.call("mgu_runs_to_labels", cuda, rp, rs, rl, B * n, off, cap, B, H, W, out, st),
                     "outlines": lambda: _lib.call("mgu_object_outlines", cuda, lab, off, cap, B, H, W, 2, B * n, 4 * B * n, lp, vp, vs, a2, st),
                     "fill": lambda: _lib.call("mgu_polygons_to_labels", cuda, lp, vp, vs, B * n, 4 * B * n, off, cap, B, H, W, 0, 2 * B * n, out, st)}
            for what, fn in calls.items():
                got.setdefault(what, set()).add(count_launches(cuda, fn))
    bits = lambda v: int(v).bit_length()  # noqa: E731
    passes = lambda nb: (nb + 7) // 8  # noqa: E731
    e = bits(4 * H * W - 1)
    assert got == {"runs": {9 + 3 * passes(bits(cap - 1))}, "paint": {1}, "outlines": {17 + e + 3 * passes(bits(cap - 1) + e)},
                   "fill": {4 + 3 * passes(bits(cap - 1) + bits(H - 1) + bits(W))}}, got


def test_invalid_arguments_return_invalid_and_launch_nothing(cuda):
    lab, off = on_device(cuda, CASES["comb"])
    z = lambda k, dt=torch.int32: torch.zeros(k, dtype=dt, device=cuda)  # noqa: E731
    ptr, st = z(2, torch.int64), z(1)
    ctx = _lib.context(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        for bad in ([None, off, 1, 1, 5, 7, 35, ptr, z(35), z(35), st], [lab, off, 1, 1, 5, 7, -1, ptr, z(35), z(35), st],
                    [lab, off, 1, 1, 5, 7, 35, ptr, None, z(35), st], [lab, off, 1, 70000, 5, 7, 35, ptr, z(35), z(35), st],
                    [lab, off, 1, 40000, 300, 300, 35, ptr, z(35), z(35), st], [lab, off, -1, 1, 5, 7, 35, ptr, z(35), z(35), st]):
            with pytest.raises(ValueError):
                _lib.call("mgu_mask_runs", cuda, *bad)
        with pytest.raises(ValueError):
            _lib.call("mgu_runs_to_labels", cuda, ptr, z(35), z(35), 35, off, 1, 1, 5, 7, None, st)
        for conn in (0, 3):
            with pytest.raises(ValueError, match="connectivity"):
                _lib.call("mgu_object_outlines", cuda, lab, off, 1, 1, 5, 7, conn, 35, 140, ptr, z(36, torch.int64), z(280), z(35, torch.int64), st)
        with pytest.raises(ValueError, match="2\\^31"):
            _lib.call("mgu_object_outlines", cuda, lab, off, 1, 6000, 300, 300, 2, 35, 140, ptr, z(36, torch.int64), z(280), z(35, torch.int64), st)
        for f in (-1, 5):
            with pytest.raises(ValueError, match="frac_bits"):
                _lib.call("mgu_polygons_to_labels", cuda, ptr, z(36, torch.int64), z(280), 35, 140, off, 1, 1, 5, 7, f, 70, lab, st)
        torch.cuda.synchronize(cuda)
        assert _lib.read_kernel_stats(ctx) == []
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    assert int(st.item()) == 0 and np.array_equal(lab.cpu().numpy(), CASES["comb"]["labels"])
    with pytest.raises(ValueError, match="connectivity"):
        mgunet.object_outlines((lab, off), 3)
    with pytest.raises(ValueError, match="frac_bits"):
        mgunet.rasterize_polygons([[]], (4, 4), frac_bits=5)


def class_map(cuda, seed, density, H=40, W=56, B=2):
    rng = np.random.default_rng(seed)
    m = (rng.random((B, H, W)) < density).astype(np.int64) * rng.integers(1, 3, (B, H, W))
    return torch.from_numpy(m).to(cuda)


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
def test_on_connected_components_and_split_objects_tables(cuda, density):
    cm = class_map(cuda, int(density * 10), density)
    for conn in (1, 2):
        table = mgunet.connected_components(cm, connectivity=conn)
        case = {"labels": table.labels.cpu().numpy(), "offsets": table.offsets.cpu().numpy()}
        runs, outl = mgunet.encode_masks(table), mgunet.object_outlines(table, conn)
        check_runs(runs, MO.encode(case["labels"], case["offsets"]))
        check_outlines(outl, MO.outlines(case["labels"], case["offsets"], conn))
        assert torch.equal(runs.areas(), table.area)
        assert torch.equal(mgunet.labels_from_runs(runs)[0], table.labels) and torch.equal(mgunet.rasterize_polygons(outl)[0], table.labels)
    blobs = torch.zeros((1, 48, 64), dtype=torch.int64, device=cuda)
    yy, xx = torch.meshgrid(torch.arange(48, device=cuda), torch.arange(64, device=cuda), indexing="ij")
    for cx, cy, r in ((14, 20, 11), (30, 22, 10), (50, 30, 9), (5, 42, 2)):
        blobs[0][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = 1
    table = mgunet.split_objects(blobs, min_distance=3, min_radius=2, min_area=int(40 * density) + 1)
    case = {"labels": table.labels.cpu().numpy(), "offsets": table.offsets.cpu().numpy()}
    check_runs(mgunet.encode_masks(table), MO.encode(case["labels"], case["offsets"]))
    check_outlines(mgunet.object_outlines(table), MO.outlines(case["labels"], case["offsets"], 2))
    assert torch.equal(mgunet.labels_from_runs(mgunet.encode_masks(table))[0].cpu(), torch.from_numpy(clean(case)))


def test_coco_dictionaries_out_and_in(cuda):
    case = CASES["scene_7x5_b3"]
    lab, off = on_device(cuda, case)
    runs = mgunet.encode_masks((lab, off))
    ptr, start, length = want_runs("scene_7x5_b3")
    plain, packed = runs.to_coco(compress=False), runs.to_coco()
    assert [len(p) for p in plain] == np.diff(case["offsets"]).tolist()
    flat = [r for per in plain for r in per]
    for i, r in enumerate(flat):
        assert r["size"] == [7, 5] and r["counts"] == MO.coco_counts(start[ptr[i]:ptr[i + 1]], length[ptr[i]:ptr[i + 1]], 35)
    assert flat[-1]["counts"] == [0, 35]                                            # the full frame ends the image: no trailing zero-run
    assert [mgunet.rle_from_string(r["counts"]) for per in packed for r in per] == [r["counts"] for r in flat]
    for rles in (plain, packed):
        back = mgunet.runs_from_coco(rles, cuda)
        check_runs(back, (ptr, start, length))
        assert back.size == (3, 7, 5) and torch.equal(back.offsets, off)
        assert np.array_equal(mgunet.labels_from_runs(back)[0].cpu().numpy(), clean(case))
    outl = mgunet.object_outlines((lab, off))
    lp, vp, v, a2 = want_outlines("scene_7x5_b3", 2)
    polys, coco = outl.to_polygons(), outl.to_coco()
    assert [len(o) for per in polys for o in per] == np.diff(lp).tolist()
    assert [len(o) for per in coco for o in per] == [int((a2[lp[i]:lp[i + 1]] > 0).sum()) for i in range(len(lp) - 1)]
    assert coco[2][0] == [[0, 0, 5, 0, 5, 7, 0, 7]]
    listed = [[(1, loops) for loops in per] for per in polys]
    assert np.array_equal(mgunet.rasterize_polygons(listed, (7, 5), device=cuda)[0].cpu().numpy(), clean(case))
    o = mgunet.object_outlines(on_device(cuda, CASES["rings_c2"]))                 # ring 1 around ring 2 around the 3 x 3 block 3
    filled = mgunet.rasterize_polygons([[(1, loops) for loops in per] for per in o.to_coco()], (11, 11), device=cuda)[0]
    want = np.ones((11, 11), np.int32)                                             # COCO polygons have no holes: the round trip fills
    want[2:9, 2:9], want[4:7, 4:7] = 2, 3                                          # every ring, and the largest label wins inside
    assert np.array_equal(filled[0].cpu().numpy(), want)


def test_to_dicts_keywords_and_downstream_on_annotations(cuda):
    gt_map, pred_map = class_map(cuda, 21, 0.6), class_map(cuda, 22, 0.55)
    gt, pred = mgunet.connected_components(gt_map, connectivity=1), mgunet.connected_components(pred_map, connectivity=1)
    runs, outl = mgunet.encode_masks(gt), mgunet.object_outlines(gt, 1)
    base = gt.to_dicts()
    assert all("segmentation" not in d for per in base for d in per)
    with_runs, with_outl, both = gt.to_dicts(runs=runs), gt.to_dicts(outlines=outl), gt.to_dicts(runs=runs, outlines=outl)
    assert both == with_runs and [[{k: v for k, v in d.items() if k != "segmentation"} for d in per] for per in with_runs] == base
    assert [[d["segmentation"] for d in per] for per in with_runs] == runs.to_coco()
    assert [[d["segmentation"] for d in per] for per in with_outl] == outl.to_coco()
    # the ground truth through COCO RLE and through polygons (with holes), as an ObjectTable again
    via_runs = mgunet.objects_from_annotations(*mgunet.labels_from_runs(mgunet.runs_from_coco(runs.to_coco(), cuda)), gt.class_id)
    via_poly = mgunet.objects_from_annotations(*mgunet.rasterize_polygons(outl), gt.class_id.tolist())
    want_ov = mgunet.object_overlaps(gt, pred)
    want_match = mgunet.match_masks(want_ov, gt, pred, thresholds=(0.5, 0.75))
    for t in (via_runs, via_poly):
        assert same(t, gt)
        ov = mgunet.object_overlaps(t, pred).check()
        n = int(want_ov.pair_ptr[-1])
        assert torch.equal(ov.pair_ptr, want_ov.pair_ptr) and torch.equal(ov.pair_gt[:n], want_ov.pair_gt[:n])
        assert torch.equal(ov.pair_inter[:n], want_ov.pair_inter[:n])
        assert all(torch.equal(a, b) for a, b in zip(mgunet.match_masks(ov, t, pred, thresholds=(0.5, 0.75)), want_match))
