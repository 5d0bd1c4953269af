"""Object splitting on the MI355X: mgu_distance_transform and mgu_split_objects BITWISE against the numpy oracle of the definitions
(split_objects_oracle.py) -- D2, seeds, labels, counts and offsets -- on shapes chosen for where the kernels can go wrong (single
pixels and lines, a width that is no multiple of 64 with two images, a row longer than a wave crossed by one component, a row past
64 KiB of LDS), the public entry points, determinism and YieldEvaluator(split=...)."""
import functools

import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
import objects_oracle as OO
import split_objects_oracle as S
from mgunet import objects

pytestmark = pytest.mark.gpu
KEYS = ("count_accuracy_perc", "yield_estimation_error_perc", "object_matching_rate_perc", "occlusion_robustness_perc",
        "total_gt_count_sum", "total_pred_count_sum")


def onehot_logits(cmap, C, dev, seed=0):
    """(B, C, H, W) view of NHWC logits whose first maximal class is cmap."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 1, tuple(cmap.shape) + (C,), generator=g).float()
    x.scatter_(-1, cmap.unsqueeze(-1), 1.0)
    return x.to(dev).permute(0, 3, 1, 2)


def assert_same(a, b):
    assert list(a) == list(KEYS) and list(b) == list(KEYS)
    for k in KEYS:
        assert np.array_equal(np.float64(a[k]).view(np.uint64), np.float64(b[k]).view(np.uint64)), (k, a[k], b[k])


def _components(cmap):
    return np.stack([OO.label(m, 2) for m in cmap])


def _scene(name):
    """int32 (B, H, W) label maps."""
    rng = np.random.default_rng(17)
    if name == "pixel":
        return np.ones((1, 1, 1))
    if name == "row7":
        return np.array([[[1, 1, 0, 2, 2, 2, 1]]])
    if name == "col7":
        return np.array([[[3], [3], [3], [0], [1], [1], [0]]])
    if name == "two_images":      # W no multiple of 64; both images use the labels 1..n: nothing may leak between them
        cmap = np.kron(rng.integers(0, 3, (2, 5, 9)), np.ones((8, 8), np.int64))[:, :37, :67]
        cmap[rng.random(cmap.shape) < 0.04] = 0
        return _components(cmap)
    if name == "square64":
        m = np.zeros((64, 64), np.int64)
        m[S.disc(m.shape, 20, 20, 12) | S.disc(m.shape, 30, 36, 12) | S.disc(m.shape, 50, 50, 9)] = 1
        m[0:6, 40:64] = 2     # touches the image border: outside pixels do not count
        return _components(m[None])
    if name == "full_width":      # one component across all 130 columns: the outward walk crosses the whole row
        m = np.zeros((40, 130), np.int64)
        m[12:27, :] = 1
        m[S.disc(m.shape, 19, 30, 14) | S.disc(m.shape, 19, 100, 16)] = 1
        return _components(m[None])
    if name == "discs":           # the scenes of the host tests
        return S.two_discs(32)[0][None]
    if name == "ellipse":
        return S.ellipse((96, 128), 48, 64, 30, 18, 0.3)[None]
    if name == "checker":
        return ((np.indices((12, 13)).sum(0) % 2) + 1)[None]
    if name == "shared_edge":     # two 7-wide labels side by side: the distance counts the other label, and their seed lines lie
        m = np.zeros((20, 30), np.int64)   # 7 pixels apart, within h of each other for r >= 13: the zones must not join
        m[2:18, 3:10], m[2:18, 10:17] = 1, 2
        return m[None]
    if name == "all_foreground":
        return np.full((1, 9, 13), 4)
    if name == "all_background":
        return np.zeros((1, 8, 8))
    if name == "line_and_bar":    # a one-pixel line (no seed) and a constant-width bar (its whole centre line is one seed group)
        m = np.zeros((40, 90), np.int64)
        m[4, 3:80] = 1
        m[12:33, 5:85] = 2
        return m[None]
    if name == "wide":            # 8200 * 8 bytes of row buffer: past 64 KiB of LDS
        m = np.zeros((2, 8200), np.int64)
        for x0 in range(0, 8200, 100):
            m[:, x0 + 3:x0 + 33] = 1 + (x0 // 100) % 5
        m[1, 4000:4400] = 9
        return m[None]
    if name == "widest":          # the documented limit: 16384 * 8 bytes = 128 KiB of LDS
        m = np.zeros((1, 16384), np.int64)
        for x0 in range(0, 16384, 128):
            m[0, x0 + 5:x0 + 36] = 1 + (x0 // 128) % 3
        m[0, 9000:9300] = 7
        return m[None]
    raise KeyError(name)


SCENES = ["pixel", "row7", "col7", "two_images", "square64", "full_width", "discs", "ellipse", "checker", "shared_edge", "all_foreground",
          "all_background", "line_and_bar"]


@functools.lru_cache(maxsize=None)
def scene(name):
    lab = np.ascontiguousarray(_scene(name), dtype=np.int32)
    lab.setflags(write=False)
    dist = np.stack([S.d2(m) for m in lab])
    dist.setflags(write=False)
    return lab, dist


def device_split(lab, r, r2, min_area, dev):
    B, H, W = lab.shape
    t = torch.from_numpy(np.array(lab)).to(dev)
    out = torch.full((B, H, W), -7, device=dev, dtype=torch.int32)
    d2 = torch.full((B, H, W), -7, device=dev, dtype=torch.int32)
    seeds = torch.full((B, H, W), 7, device=dev, dtype=torch.uint8)
    counts = torch.full((B,), -7, device=dev, dtype=torch.int64)
    offsets = torch.full((B + 1,), -7, device=dev, dtype=torch.int64)
    objects._split(t, B, H, W, (r, r2, min_area), out, counts, offsets, d2, seeds)
    return d2.cpu().numpy(), seeds.cpu().numpy(), out.cpu().numpy(), counts.cpu().numpy(), offsets.cpu().numpy()


def check_bitwise(got, want, tag):
    for g, w, what in zip(got, want, ("d2", "seeds", "labels", "counts", "offsets")):
        assert g.shape == w.shape and np.array_equal(g, w.astype(g.dtype)), (tag, what)


@pytest.mark.parametrize("name", SCENES)
def test_distance_transform_bitwise(cuda, name):
    lab, dist = scene(name)
    got = mgunet.distance_transform(torch.from_numpy(np.array(lab)).to(cuda))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), dist)


def test_distance_transform_takes_any_int32_label(cuda):
    lab = np.array(scene("shared_edge")[0])
    lab[lab == 2] = -5
    lab[lab == 1] = 2 ** 31 - 1
    got = mgunet.distance_transform(torch.from_numpy(lab).to(cuda)[0])   # an (H, W) map is a batch of one
    assert np.array_equal(got.cpu().numpy(), scene("shared_edge")[1])


@pytest.mark.parametrize("r", [1, 3, 8, 16])
@pytest.mark.parametrize("name", SCENES)
def test_split_bitwise(cuda, name, r):
    lab, dist = scene(name)
    for min_area in (0, 30):
        want = S.split_batch(lab, r, 9, min_area, dist=dist)
        check_bitwise(device_split(lab, r, 9, min_area, cuda), want, (name, r, min_area))
    if name == "line_and_bar":
        seeds, out = want[1][0], want[2][0]
        assert not seeds[4].any() and seeds[22, 15:75].all() and len(np.unique(out[lab[0] == 2])) == 1
    if name == "shared_edge" and r == 16:
        assert want[3][0] == 2 and want[1][0][:, 6].any() and want[1][0][:, 13].any()
    if name == "all_background":
        assert want[3][0] == 0
    if name in ("discs", "ellipse") and r <= 8:
        assert want[3].tolist() == [2 if name == "discs" else 1]


def test_split_wide_row_and_other_radius(cuda):
    for name in ("wide", "widest", "wide"):   # rows past 64 KiB of LDS in increasing width, then back, in one process
        lab, dist = scene(name)
        check_bitwise(device_split(lab, 3, 9, 0, cuda), S.split_batch(lab, 3, 9, 0, dist=dist), name)
    got = mgunet.distance_transform(torch.from_numpy(np.array(scene("widest")[0])).to(cuda))
    assert np.array_equal(got.cpu().numpy(), scene("widest")[1])
    lab, dist = scene("square64")
    for r2 in (1, 50, 200):
        check_bitwise(device_split(lab, 5, r2, 0, cuda), S.split_batch(lab, 5, r2, 0, dist=dist), ("square64", r2))


def test_split_in_place_and_without_optional_outputs(cuda):
    lab, dist = scene("square64")
    want = S.split_batch(lab, 5, 9, 30, dist=dist)
    t = torch.from_numpy(np.array(lab)).to(cuda)
    counts = torch.empty(1, device=cuda, dtype=torch.int64)
    offsets = torch.empty(2, device=cuda, dtype=torch.int64)
    objects._split(t, 1, 64, 64, (5, 9, 30), t, counts, offsets)
    assert np.array_equal(t.cpu().numpy(), want[2]) and counts.tolist() == want[3].tolist() and offsets.tolist() == want[4].tolist()


def test_determinism(cuda):
    lab, _ = scene("discs")
    a = device_split(lab, 5, 9, 0, cuda)
    b = device_split(lab, 5, 9, 0, cuda)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def _class_scene():
    cmap = np.zeros((2, 48, 160), np.int64)
    cmap[0] = S.touching_pairs()[0]
    cmap[1, S.disc((48, 160), 20, 40, 12) | S.disc((48, 160), 26, 56, 12)] = 2
    cmap[1, 5:9, 100:150] = 1
    return cmap


def test_entry_points_agree_and_stats_match_the_oracle(cuda):
    cmap = _class_scene()
    t = torch.from_numpy(cmap).to(cuda)
    kw = dict(min_distance=5, min_radius=3, min_area=20)
    a, seeds = mgunet.split_objects(t, return_seeds=True, **kw)
    b = mgunet.split_objects(onehot_logits(torch.from_numpy(cmap), 3, cuda), **kw)
    c = mgunet.split_objects(mgunet.connected_components(t), **kw)
    comp = _components(cmap)
    d2w, seedw, labw, cntw, offw = S.split_batch(comp, 5, 9, 20)
    assert seeds.dtype == torch.bool and np.array_equal(seeds.cpu().numpy(), seedw)
    assert cntw.tolist() == [6, 3]
    stats = [OO.stats(labw[i], cmap[i]) for i in range(2)]
    for tab in (a, b, c):
        assert np.array_equal(tab.labels.cpu().numpy(), labw) and tab.labels.dtype == torch.int32
        assert tab.counts.tolist() == cntw.tolist() and tab.offsets.tolist() == offw.tolist()
        for k, field in enumerate((tab.class_id, tab.area, tab.bbox, tab.sums)):
            assert np.array_equal(field.cpu().numpy(), np.concatenate([s[k] for s in stats])), k
    single = mgunet.split_objects(t[1], **kw)
    assert np.array_equal(single.labels.cpu().numpy(), labw[1:2]) and single.counts.tolist() == [3]
    empty = mgunet.split_objects(torch.zeros((1, 8, 8), dtype=torch.int64, device=cuda))
    assert empty.counts.tolist() == [0] and empty.area.numel() == 0


def test_yield_evaluator_split(cuda):
    n = 3
    cmap = torch.from_numpy(S.touching_pairs(n)[0])[None]
    logits = onehot_logits(cmap, 2, cuda)
    plain, default = mgunet.YieldEvaluator(2, cuda), mgunet.YieldEvaluator(2, cuda, split=None)
    for ev in (plain, default):
        ev.update(logits, cmap.to(cuda))
    assert_same(plain.compute(), default.compute())
    assert plain.compute()["total_pred_count_sum"] == n
    ev = mgunet.YieldEvaluator(2, cuda, split={"min_distance": 5, "min_radius": 3})
    ev.update(logits, cmap.to(cuda))
    assert_same(ev.compute(), S.touching_pairs_expected(n))
    with pytest.raises(ValueError):
        mgunet.YieldEvaluator(2, cuda, split={"connectivity": 1})


def test_evaluate_yield_split_equals_the_evaluator(cuda):
    cfg = (3, 2, 8, 2)
    model = mgunet.UNet(*cfg)
    model.load_state_dict(O.make_unet_params(*cfg, seed=9))
    model = model.to(cuda).eval()
    g = torch.Generator().manual_seed(5)
    masks = torch.from_numpy(S.touching_pairs(1, shape=(48, 64))[0])
    loader = [(torch.randn((b, 3, 48, 64), generator=g), masks[None].repeat(b, 1, 1)) for b in (2, 1)]
    split = {"min_distance": 3, "min_radius": 2, "min_area": 4}
    res = mgunet.evaluate_yield(model, loader, split=split)
    ev = mgunet.YieldEvaluator(2, cuda, split=split)
    with torch.no_grad():
        for x, y in loader:
            ev.update(model(x.to(cuda))[0], y.to(cuda))
    assert_same(res, ev.compute())
    assert res["total_gt_count_sum"] == 6   # three images of one touching pair, each split in two
    plain = mgunet.evaluate_yield(model, loader)
    assert plain["total_gt_count_sum"] == 3
