"""Every user of csrc/objects_common.h's wave_by_key at every fill level of a wave, on the MI355X: cc_flatten_kernel (min_area),
stats_kernel, scores_kernel, moments_kernel, residual_kernel and panoptic_kernel's class_add, plus the two chunk scans the header's
chunk_sum_scan serves.  Expected values come from the numpy oracles (objects_oracle, shapes_oracle, instances_oracle); integers are
compared bit for bit, the shape floats as test_gpu_shapes.py compares them (1 fp32 ulp).

Inputs: int64 class maps of 2 x 16 x 200 -- W is no multiple of 64, so waves straddle rows, and of the 25 workgroups of 256 pixels one
straddles the two images -- made of vertical stripes of width w whose classes cycle 1..6 (image 1: three classes on, its first 5
columns background), so neighbouring stripes never join and a wave meets more than 4 classes:
  w = 1    64 objects per wave, every object a one-pixel-wide line: the per-pixel residual route
  w = 13   5 objects per wave: the first lane past the 4 grouped keys adds directly
  w = 16   4 to 5 objects per wave, around the group count
  w = 200  one object per image: everything in the first group
and a 4-connectivity checkerboard over six classes: 3200 one-pixel objects in one 16 x 200 image, through every chunk of both scans."""
import functools

import numpy as np
import pytest
import torch

import instances_oracle as IO
import mgunet
import objects_oracle as OO
import shapes_oracle as SO
from mgunet import objects as mobj
from test_gpu_shapes import check_object, host

pytestmark = pytest.mark.gpu

H, W, C = 16, 200, 7
CASES = ["w1", "w13", "w16", "w200", "checker"]


def class_maps(name):
    """(int64 maps (B, H, W), connectivity)"""
    x = np.arange(W)
    if name == "checker":
        return ((x[None, :] + np.arange(H)[:, None]) % 6 + 1)[None].astype(np.int64), 1
    w = int(name[1:])
    m = np.stack([np.broadcast_to((x // w + shift) % 6 + 1, (H, W)) for shift in (0, 3)]).astype(np.int64)
    m[1, :, :5] = 0
    return m, 2


def shifted(m):
    """the maps one column to the right, column 0 background"""
    out = np.zeros_like(m)
    out[:, :, 1:] = m[:, :, :-1]
    return out


def power_sums(lab, bbox):
    """int64 (n, 12): sum of x^2 xy y^2 | x^3 x^2y xy^2 y^3 | x^4 x^3y x^2y^2 xy^3 y^4 over every object's pixels, coordinates taken
    from the object's (xmin, ymin) -- what mgu_object_moments accumulates (exact in int64 at these sizes)."""
    ys, xs = np.nonzero(lab)
    k = lab[ys, xs].astype(np.int64) - 1
    x, y = xs - bbox[k, 0], ys - bbox[k, 1]
    terms = [x * x, x * y, y * y, x ** 3, x * x * y, x * y * y, y ** 3, x ** 4, x ** 3 * y, x * x * y * y, x * y ** 3, y ** 4]
    return np.stack([np.bincount(k, t, minlength=len(bbox)).astype(np.int64) for t in terms], 1)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Everything the tests of one input expect, computed once: the labelling and the per-object arrays of the map and of the map
    shifted one column, batch-wide row order."""
    m, conn = class_maps(name)
    out = {"maps": m, "conn": conn}
    for side, maps in (("gt", m), ("pred", shifted(m))):
        labels = np.stack([OO.label(v, conn) for v in maps])
        per_image = [OO.stats(lab, v) for lab, v in zip(labels, maps)]
        cls, area, bbox, sums = (np.concatenate([s[k] for s in per_image]) for k in range(4))
        out[side] = {"labels": labels, "offsets": IO.offsets_of(labels), "cls": cls, "area": area, "bbox": bbox, "sums": sums}
    return out


def device_table(cuda, maps, conn, min_area=0):
    return mgunet.connected_components(torch.from_numpy(maps).to(cuda), connectivity=conn, min_area=min_area)


def check_table(t, want):
    assert t.labels.dtype == torch.int32 and np.array_equal(t.labels.cpu().numpy(), want["labels"])
    assert np.array_equal(t.offsets.cpu().numpy(), want["offsets"])
    assert np.array_equal(t.counts.cpu().numpy(), np.diff(want["offsets"]))
    for got, key in ((t.class_id, "cls"), (t.area, "area"), (t.bbox, "bbox"), (t.sums, "sums")):
        assert np.array_equal(got.cpu().numpy(), want[key]), key


@pytest.mark.parametrize("name", CASES)
def test_labels_and_statistics(cuda, name):
    o = oracle(name)
    t0, t1 = (device_table(cuda, o["maps"], o["conn"], a) for a in (0, 1))
    check_table(t0, o["gt"])
    for f in ("labels", "counts", "offsets", "class_id", "area", "bbox", "sums"):   # min_area 1 drops nothing: the same bits
        assert torch.equal(getattr(t0, f), getattr(t1, f)), f
    if name == "checker":
        assert t0.counts.tolist() == [H * W]
    else:
        w = int(name[1:])
        assert t0.counts.tolist() == [-(-W // w), -(-W // w) - (5 // w)]


@pytest.mark.parametrize("name", CASES)
def test_object_scores(cuda, name):
    """the fixed-point sum of mgu_object_scores restated on the oracle's objects: sum of round_half_even(p * 2^32) per object in
    uint64, (sum * 2^-32) / area in float64, rounded to float32"""
    o = oracle(name)
    want, B = o["gt"], len(o["maps"])
    probs = torch.rand((B, C, H, W), generator=torch.Generator().manual_seed(7))
    got = mgunet.object_scores(device_table(cuda, o["maps"], o["conn"]), probs.to(cuda)).cpu().numpy()
    bs, ys, xs = np.nonzero(want["labels"])
    obj = want["offsets"][bs] + want["labels"][bs, ys, xs] - 1
    p = probs.numpy()[bs, want["cls"][obj], ys, xs]
    acc = np.zeros(len(want["cls"]), np.uint64)
    np.add.at(acc, obj, np.rint(p.astype(np.float64) * 2.0 ** 32).astype(np.uint64))
    ref = ((acc.astype(np.float64) * 2.0 ** -32) / want["area"].astype(np.float64)).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", CASES)
def test_object_shapes(cuda, name):
    o = oracle(name)
    want, B = o["gt"], len(o["maps"])
    t = device_table(cuda, o["maps"], o["conn"])
    N = t.area.numel()
    moments = torch.empty((N, 12), device=cuda, dtype=torch.int64)
    out = mobj._shapes(t.labels, B, H, W, t.offsets, N, t.area, t.bbox, t.sums, 1e-6, 10, moments=moments)
    sh = mgunet.ObjectShapes(*out, t.offsets, t.class_id)
    sums = np.concatenate([power_sums(lab, want["bbox"][a:b]) for lab, a, b in zip(want["labels"], want["offsets"], want["offsets"][1:])])
    assert np.array_equal(moments.cpu().numpy(), sums)
    shapes = [s for lab in want["labels"] for s in SO.shapes_of_labels(lab)]
    h = host(sh)
    assert len(h["status"]) == len(shapes)
    analysed = sum(check_object(h, i, s, (name, i))[0] for i, s in enumerate(shapes))
    assert analysed == (0 if name == "checker" else len(shapes))
    if analysed:   # the device averages terms already rounded to fp32 and rounds once more (test_gpu_shapes.py): 2 ulp of the largest
        assert abs(float(sh.loss()) - SO.loss(shapes)) <= 2.0 * SO.ulp32(max(s["term"] for s in shapes))
    else:
        assert float(sh.loss()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_matching_against_the_shifted_map(cuda, name):
    o = oracle(name)
    g, p = o["gt"], o["pred"]
    tg, tp = (device_table(cuda, m, o["conn"]) for m in (o["maps"], shifted(o["maps"])))
    check_table(tp, p)
    table = mgunet.object_overlaps(tg, tp).check()
    ov = IO.overlaps(g["labels"], p["labels"])
    k = ov["pairs"]
    assert ov["status"] == 0 and np.array_equal(table.pair_ptr.cpu().numpy(), ov["pair_ptr"])
    assert np.array_equal(table.pair_gt[:k].cpu().numpy(), ov["pair_gt"]) and np.array_equal(table.pair_inter[:k].cpu().numpy(), ov["pair_inter"])
    words, _ = IO.panoptic(g["labels"], p["labels"], g["cls"], p["cls"], C)
    assert np.array_equal(mgunet.panoptic_totals(table, tg, tp, C).cpu().numpy().view(np.uint64), words)
    mg, mi, totals = IO.match(g["labels"], p["labels"], g["cls"], p["cls"], [0.5])
    dmg, dmi, dtotals = mgunet.match_masks(table, tg, tp, (0.5,))
    assert np.array_equal(dmg.cpu().numpy(), mg) and np.array_equal(dmi.cpu().numpy().view(np.uint64), mi.view(np.uint64))
    assert np.array_equal(dtotals.cpu().numpy(), totals)
