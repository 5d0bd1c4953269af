"""Boundary evaluation on the MI355X: the three tables of mgunet.boundary_tables BITWISE against the scipy oracle of the definitions
(boundary_oracle.py) on shapes chosen for where the column and row passes can go wrong (single pixels and lines, widths around the
64-lane column block, a row wider than a 256-thread workgroup, several images), class maps and logits with ties, junk values on both
sides, both histogram sizes and four band radii; hand-built scenes; symmetry, determinism and the empty batch; the evaluator against
boundary_metrics of the oracle's tables; and the distance transform and the split, whose host helper moved, against their oracles."""
import functools

import numpy as np
import pytest
import torch

import boundary_oracle as K
import mgunet
import mgunet_oracle as O
import split_objects_oracle as S
from mgunet import objects

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (1, 1, 70), (2, 37, 1), (2, 37, 63), (2, 37, 64), (2, 37, 65), (3, 61, 131), (1, 40, 300)]
RADIUS = {1: 1, 4: 2, 25: 5, 64: 8}                      # a band radius whose floor(radius^2) is band_r2


@functools.lru_cache(maxsize=None)
def pair(shape, C, seed=3):
    out = K.blob_pair(shape, C, seed)
    for a in out:
        a.setflags(write=False)
    return out


def dev_tables(pred, target, dev, num_classes=None, **kw):
    to = lambda a: a.to(dev) if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    t = mgunet.boundary_tables(to(pred), to(target), num_classes, **kw)
    assert all(x.dtype == torch.int64 and x.is_cuda for x in (t.hist, t.stats, t.band))
    return t


def as_numpy(t):
    return mgunet.BoundaryTables(t.hist.cpu().numpy(), t.stats.cpu().numpy(), t.band.cpu().numpy(), t.max_d2, t.band_r2)


def check(pred, target, dev, C, max_distance=64, band_r2=4, pred_map=None):
    """device tables of (pred, target) == oracle tables of (pred_map or pred, target); returns the device tables as numpy"""
    max_d2 = K.radius_sq(max_distance)
    ref = K.tables(pred if pred_map is None else pred_map, target, C, max_d2, band_r2)
    got = as_numpy(dev_tables(pred, target, dev, None if pred_map is not None else C, max_distance=max_distance, band_radius=RADIUS[band_r2]))
    assert (got.max_d2, got.band_r2) == (max_d2, band_r2)
    for g, r, what in zip((got.hist, got.stats, got.band), ref, ("hist", "stats", "band")):
        assert g.shape == r.shape and np.array_equal(g, r), (what, np.argwhere(g != r)[:8])
    return got


def nchw_view(planes, dev):
    """the NCHW view of NHWC storage, as UNet.forward returns its logits"""
    return torch.from_numpy(np.array(planes)).to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tables_bitwise_every_shape(cuda, shape, C):
    planes, pred, target = pair(shape, C)
    check(pred, target, cuda, C, max_distance=8, band_r2=1)
    check(pred, target, cuda, C, max_distance=64, band_r2=25)
    cmap = K.argmax_first(planes)                        # ties between classes occur: the first maximal class
    assert np.array_equal(cmap, torch.argmax(torch.from_numpy(np.array(planes)).to(cuda), 1).cpu().numpy())
    check(nchw_view(planes, cuda), target, cuda, C, max_distance=8, band_r2=4, pred_map=cmap)
    check(torch.from_numpy(np.array(planes)), target, cuda, C, max_distance=64, band_r2=64, pred_map=cmap)   # NCHW storage


def test_planes_hold_ties_and_maps_hold_junk():
    planes, pred, target = pair((3, 61, 131), 3)
    top = np.sort(planes, axis=1)
    assert (top[:, -1] == top[:, -2]).any()
    for m in (pred, target):
        assert (m == -100).any() and (m == 6).any()


def test_overflow_bin_is_reached(cuda):
    """at (1, 40, 300), C = 3, max_distance = 8 the pair puts boundary pixels farther than 8 from the other side's: the walk past the
    histogram's range and the overflow bin are exercised"""
    _, pred, target = pair((1, 40, 300), 3)
    got = check(pred, target, cuda, 3, max_distance=8, band_r2=4)
    assert got.hist[..., -1].sum() > 0 and got.stats[..., 1].sum() == 0   # all matched, some beyond max_d2
    assert got.stats[..., 2].max() > 64


def test_widest_row_takes_the_large_lds_path(cuda):
    """W = 16384 with the full histogram: 80 KiB of LDS per workgroup, past the 64 KiB a kernel gets without asking; then a narrow
    call again in the same process"""
    _, pred, target = pair((1, 3, 16384), 2)
    got = check(pred, target, cuda, 2, max_distance=64, band_r2=4)
    assert got.stats[..., 0].sum() > 1000
    _, pred, target = pair((2, 37, 65), 2)
    check(pred, target, cuda, 2, max_distance=64, band_r2=4)


def test_two_squares(cuda):
    p, g = K.two_squares()
    got = check(p, g, cuda, 2, max_distance=4, band_r2=4)
    for d in (0, 1):
        assert got.stats[0, 0, d].tolist() == [28, 0, 9, 2752512]
        assert {k: int(v) for k, v in enumerate(got.hist[0, 0, d]) if v} == {0: 10, 1: 4, 4: 4, 9: 10}
    assert got.band[0, 0].tolist() == [20, 48, 48]
    m = mgunet.boundary_metrics(got, tolerance=1.0)
    assert m["hausdorff"] == [3.0] and m["assd"] == [1.5] and m["bf_score"] == [0.5] and m["boundary_iou"] == [20 / 76]


def test_hand_scenes(cuda):
    H, W = 24, 300
    p, g = np.zeros((6, H, W), np.int64), np.zeros((6, H, W), np.int64)
    p[0, 4:10, 5:20] = 1                                 # class 1 on the prediction only; class 2 on neither side
    p[1, 0:8, 0:9], g[1, 0:8, 0:12] = 1, 1               # touching the frame: no boundary along the frame
    p[2, 5:15, 10:20], p[2, 5:15, 20:30] = 1, 2          # two classes sharing an edge: both rims are boundary
    g[2, 5:15, 10:22], g[2, 5:15, 22:30] = 1, 2
    p[3, 3, 3], p[3, 20, 290], g[3, 3, 5], g[3, 10, 150] = 1, 1, 1, 1   # single-pixel objects
    p[4, 12, 0], g[4, 12, 299] = 2, 2                    # the only site at the far end of the row
    p[5], g[5] = 1, 1                                    # entirely one class
    g[5, 10:14, 100:104] = 0
    for max_distance in (8, 64):
        got = check(p, g, cuda, 3, max_distance=max_distance, band_r2=4)
    assert got.stats[0, 0, 0].tolist() == [38, 38, 0, 0] and got.hist[0, 0, 0, -1] == 38 and not got.stats[0, 0, 1].any()
    assert not got.stats[0, 1].any() and not got.hist[0, 1].any() and not got.band[0, 1].any()
    assert got.stats[1, 0, :, 0].tolist() == [8 + 9 - 1, 8 + 12 - 1]   # the right column and the bottom row, the corner pixel once
    assert got.stats[2, 0, 0, 0] == 36 and got.stats[2, 1, 0, 0] == 36 and got.stats[2, 0, 0, 2] == 4
    assert got.stats[3, 0, 0].tolist()[:3] == [2, 0, 140 ** 2 + 10 ** 2] and got.stats[3, 0, 1, 2] == 140 ** 2 + 10 ** 2
    assert got.stats[4, 1, 0].tolist() == [1, 0, 299 ** 2, 299 * 65536] and got.hist[4, 1, 0, -1] == 1
    assert got.stats[5, 0, 0].tolist() == [0, 0, 0, 0] and got.stats[5, 0, 1].tolist() == [16, 16, 0, 0]
    assert got.band[5, 0].tolist() == [0, 0, 4 * 4 * 2 + 4 * 1]   # D2 <= 4 around the 4 x 4 hole: two rings along each side, one pixel at each corner; the full map has no band


def test_identical_maps(cuda):
    _, pred, _ = pair((3, 61, 131), 4)
    got = check(pred, pred, cuda, 4, max_distance=8, band_r2=4)
    assert got.hist[..., 1:].sum() == 0 and got.stats[..., 1:].sum() == 0 and got.stats[..., 0].sum() > 0
    assert np.array_equal(got.band[..., 0], got.band[..., 1]) and np.array_equal(got.band[..., 0], got.band[..., 2])
    m = mgunet.boundary_metrics(got)
    assert m["bf_score"] == [1.0] * 3 and m["boundary_iou"] == [1.0] * 3 and m["hausdorff"] == [0.0] * 3 and m["assd"] == [0.0] * 3


def test_swapping_the_sides_swaps_the_directions(cuda):
    _, pred, target = pair((2, 37, 65), 3)
    a = as_numpy(dev_tables(pred, target, cuda, 3, max_distance=8, band_radius=2))
    b = as_numpy(dev_tables(target, pred, cuda, 3, max_distance=8, band_radius=2))
    assert np.array_equal(a.hist, b.hist[:, :, ::-1]) and np.array_equal(a.stats, b.stats[:, :, ::-1])
    assert np.array_equal(a.band, b.band[:, :, [0, 2, 1]])
    ma, mb = mgunet.boundary_metrics(a), mgunet.boundary_metrics(b)
    assert ma["bf_precision"] == mb["bf_recall"] and ma["bf_score"] == mb["bf_score"] and ma["hd95"] == mb["hd95"]


def test_repeatable_batch_of_one_and_empty_batch(cuda):
    _, pred, target = pair((3, 61, 131), 3)
    a = as_numpy(dev_tables(pred, target, cuda, 3))
    b = as_numpy(dev_tables(pred, target, cuda, 3))
    for x, y in zip((a.hist, a.stats, a.band), (b.hist, b.stats, b.band)):
        assert np.array_equal(x, y)
    assert a.max_d2 == 4096 and a.band_r2 == K.default_band_r2(61, 131)
    one = as_numpy(dev_tables(pred[1], target[1], cuda, 3))   # an (H, W) input is a batch of one
    assert one.hist.shape == (1, 2, 2, 4098) and np.array_equal(one.hist[0], a.hist[1]) and np.array_equal(one.stats[0], a.stats[1])
    assert np.array_equal(one.band[0], a.band[1])
    e = dev_tables(np.zeros((0, 4, 4), np.int64), np.zeros((0, 4, 4), np.int64), cuda, 3, max_distance=2)
    assert tuple(e.hist.shape) == (0, 2, 2, 6) and tuple(e.stats.shape) == (0, 2, 2, 4) and tuple(e.band.shape) == (0, 2, 3)
    z = dev_tables(np.zeros((2, 0, 4), np.int64), np.zeros((2, 0, 4), np.int64), cuda, 2, max_distance=2)
    assert tuple(z.hist.shape) == (2, 1, 2, 6) and not z.hist.any() and not z.stats.any() and not z.band.any()


def onehot_logits(cmap, C, dev, seed=0):
    """(B, C, H, W) view of NHWC logits whose first maximal class is cmap"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 1, tuple(cmap.shape) + (C,), generator=g).float()
    x.scatter_(-1, cmap.unsqueeze(-1), 1.0)
    return x.to(dev).permute(0, 3, 1, 2)


def test_evaluator_equals_metrics_of_the_oracle_tables(cuda):
    C, shape = 3, (6, 37, 65)
    planes, _, target = pair(shape, C, 8)
    cmap = K.argmax_first(planes)
    target = np.array(target)
    target[4][target[4] == 2] = 0                        # an image whose class 2 is on the prediction only
    ev = mgunet.BoundaryEvaluator(C, cuda, tolerance=1.5, max_distance=8, band_radius=2, quantile=0.9)
    for lo, hi in ((0, 3), (3, 4), (4, 6)):              # three batches of different B
        ev.update(nchw_view(planes[lo:hi], cuda), torch.from_numpy(target[lo:hi]).to(cuda))
    ref = mgunet.BoundaryTables(*K.tables(cmap, target, C, 64, 4), 64, 4)
    want = mgunet.boundary_metrics(ref, tolerance=1.5, quantile=0.9)
    got = ev.compute()
    assert got == want and list(got) == list(want)
    assert got["missing"][1] >= 1 and got["images"][0] >= 1
    t = ev.tables()
    assert np.array_equal(t.hist.cpu().numpy(), ref.hist) and t.band_r2 == 4
    ev.reset()
    assert ev.compute()["images"] == [0, 0]


def test_evaluate_boundaries_equals_the_evaluator_fed_by_hand(cuda):
    cfg = (3, 2, 8, 2)
    model = mgunet.UNet(*cfg)
    model.load_state_dict(O.make_unet_params(*cfg, seed=9))
    model = model.to(cuda).eval()
    g = torch.Generator().manual_seed(5)
    masks = torch.from_numpy(K.two_squares()[0][0]).repeat(4, 3)[:64, :64]
    loader = [(torch.randn((b, 3, 64, 64), generator=g), masks[None].repeat(b, 1, 1)) for b in (2, 1)]
    kw = dict(tolerance=1.0, max_distance=16, quantile=0.95)
    ev = mgunet.BoundaryEvaluator(2, cuda, **kw)
    with torch.no_grad():
        for x, y in loader:
            ev.update(model(x.to(cuda))[0], y.to(cuda))
    got = mgunet.evaluate_boundaries(model, loader, **kw)
    assert got == ev.compute() and len(got["bf_score"]) == 1


def test_distance_transform_and_split_unchanged(cuda):
    """the distance transform's host helper is now shared with boundary.hip: both of its callers still equal their oracles"""
    _, pred, _ = pair((2, 37, 65), 3)
    table = mgunet.connected_components(torch.from_numpy(K.normalise(pred, 3)).to(cuda))
    lab = table.labels.cpu().numpy()
    dist = np.stack([S.d2(m) for m in lab])
    assert np.array_equal(mgunet.distance_transform(table).cpu().numpy(), dist)
    B, H, W = lab.shape
    out, counts, offsets = torch.empty_like(table.labels), torch.empty(B, device=cuda, dtype=torch.int64), torch.empty(B + 1, device=cuda, dtype=torch.int64)
    d2 = torch.empty_like(table.labels)
    seeds = torch.empty((B, H, W), device=cuda, dtype=torch.uint8)
    objects._split(table.labels, B, H, W, (3, 4, 0), out, counts, offsets, d2, seeds)
    want = S.split_batch(lab, 3, 4, 0, dist=dist)
    for got, w in zip((d2, seeds, out, counts, offsets), want):
        assert np.array_equal(got.cpu().numpy(), w.astype(got.cpu().numpy().dtype))


def test_bad_arguments_raise(cuda):
    m = torch.zeros((1, 8, 8), dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError):
        mgunet.boundary_tables(m, m)                     # a class map needs num_classes
    for n in (1, 33):
        with pytest.raises(ValueError):
            mgunet.boundary_tables(m, m, n)
    with pytest.raises(ValueError):
        mgunet.boundary_tables(m, m[:, :4], 2)
    with pytest.raises(ValueError):
        mgunet.boundary_tables(torch.zeros((1, 3, 8, 8), device=cuda), m, 2)   # logits of 3 classes
    with pytest.raises(TypeError):
        mgunet.boundary_tables(m, m.float(), 2)
    with pytest.raises(RuntimeError):
        mgunet.boundary_tables(m, m.cpu(), 2)
    h, s, b = (torch.zeros(n, dtype=torch.int64, device=cuda) for n in (2 * 6, 2 * 4, 3))
    good = (m, 0, m, 1, 8, 8, 0, 2, 4, 1, h, s, b)
    mgunet._lib.call("mgu_boundary_tables", cuda, *good)
    for i, v in ((1, 2), (7, 1), (7, 33), (8, 0), (8, 4097), (9, 0), (0, None), (2, None), (10, None), (11, None), (12, None), (3, -1)):
        args = list(good)
        args[i] = v
        with pytest.raises(ValueError):                  # the C entry point: kind, num_classes, max_d2, band_r2, null pointers, size
            mgunet._lib.call("mgu_boundary_tables", cuda, *args)
    with pytest.raises(ValueError):                      # logits whose channels are not num_classes
        mgunet._lib.call("mgu_boundary_tables", cuda, torch.zeros((1, 8, 8, 3), device=cuda), 1, m, 1, 8, 8, 3, 2, 4, 1, h, s, b)
