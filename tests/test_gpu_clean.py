"""Mask cleanup on the MI355X: mgunet.clean_masks BITWISE against the scipy oracle of the definition (clean_oracle.py), result and
counts, on shapes chosen for where the bit-plane kernels can go wrong (single pixels and lines, widths around the 64-pixel word and
the 128-pixel tile, heights around the 32-row tile, several images), every disc from r2 = 1 to 64, logits and class maps, hand-built
scenes for the fill rules, determinism, idempotence of the single stages, the pin-hole table of split_objects end to end, and the
clean= option of the two object evaluators against the composition of the public functions."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import clean_oracle as K
import mgunet
import mgunet_oracle as O

pytestmark = pytest.mark.gpu
R2S = (1, 2, 4, 5, 8, 9, 64)
SHAPES = [(1, 1, 1), (1, 1, 70), (2, 37, 1), (2, 37, 63), (2, 37, 64), (2, 37, 65), (1, 37, 130), (3, 37, 70), (2, 61, 131)]
RADIUS = {1: 1, 2: 1.5, 4: 2, 5: 2.3, 8: 2.9, 9: 3, 64: 8}      # a radius whose floor(radius^2) is r2
YKEYS = ("count_accuracy_perc", "yield_estimation_error_perc", "object_matching_rate_perc", "occlusion_robustness_perc",
         "total_gt_count_sum", "total_pred_count_sum")


@functools.lru_cache(maxsize=None)
def blob_planes(shape, C, seed):
    """(B, C, H, W) smooth noise planes, quantised so that ties between classes occur; class 0 is slightly favoured"""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    x = np.stack([[ndimage.gaussian_filter(rng.standard_normal((H, W)), 2.5, mode="constant") for _ in range(C)] for _ in range(B)])
    x[:, 0] += 0.02
    x = np.round(x * 16) / 16 + (rng.random(x.shape) < 0.03) * rng.integers(-1, 2, x.shape) * 0.5
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def blob_map(shape, C, seed):
    """int64 (B, H, W) blob class map of C classes, with -100 and out-of-range values sprinkled in"""
    m = K.argmax_first(blob_planes(shape, C, seed))
    rng = np.random.default_rng(seed + 100)
    junk = rng.random(m.shape)
    m[junk < 0.01] = -100
    m[(junk >= 0.01) & (junk < 0.02)] = C + 3
    m.setflags(write=False)
    return m


def run(x, dev, num_classes=None, **kw):
    x = x.clone() if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x))   # a copy: the cached maps are read-only
    out, counts = mgunet.clean_masks(x.to(dev), num_classes, return_counts=True, **kw)
    assert out.dtype == torch.int64 and counts.dtype == torch.int64
    return out.cpu(), counts.cpu()


def check(x, dev, num_classes, close_r2=0, fill_holes=True, max_hole_area=0, open_r2=0):
    ref, refc = K.clean(x, num_classes, close_r2, fill_holes, max_hole_area, open_r2)
    out, counts = run(x, dev, num_classes, close_radius=RADIUS.get(close_r2, 0), fill_holes=fill_holes, max_hole_area=max_hole_area,
                      open_radius=RADIUS.get(open_r2, 0))
    assert tuple(out.shape) == ref.shape
    assert torch.equal(out, torch.from_numpy(ref)), np.argwhere(out.numpy() != ref)[:8]
    assert torch.equal(counts, torch.from_numpy(refc)), (counts, refc)
    return out, counts


def test_radii_square_as_documented():
    assert [K.radius_sq(RADIUS[r2]) for r2 in R2S] == list(R2S)


@pytest.mark.parametrize("r2", R2S)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_class_maps_every_shape_and_disc(cuda, shape, r2):
    m = blob_map(shape, 3, 11)
    check(m, cuda, 3, close_r2=r2, fill_holes=False)
    check(m, cuda, 3, fill_holes=False, open_r2=r2)
    check(m, cuda, 3, close_r2=r2, fill_holes=True, open_r2=r2)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_blob_maps_stage_by_stage(cuda, seed):
    m = blob_map((2, 61, 131), 3, seed)
    check(m, cuda, 3)                                    # fill only
    check(m, cuda, 3, max_hole_area=3)
    check(m, cuda, 3, close_r2=4, open_r2=2)
    check(m, cuda, 3, close_r2=2, open_r2=9, max_hole_area=12)
    check(m, cuda, 3, fill_holes=False)                  # no stage: the class map, background as 0


@pytest.mark.parametrize("C", [2, 4])
def test_logits_argmax_fused(cuda, C):
    shape = (3, 37, 70)
    x = np.array(blob_planes(shape, C, 5 + C))
    cmap = K.argmax_first(x)
    dev_arg = torch.argmax(torch.from_numpy(x).to(cuda), 1).cpu().numpy()
    assert np.array_equal(cmap, dev_arg)
    logits = torch.from_numpy(x).to(cuda).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # the NCHW view of NHWC storage
    for kw in ({"close_r2": 2, "open_r2": 2}, {"close_r2": 5, "fill_holes": False}, {"open_r2": 4}, {}):
        ref, refc = K.clean(cmap, C, kw.get("close_r2", 0), kw.get("fill_holes", True), 0, kw.get("open_r2", 0))
        out, counts = mgunet.clean_masks(logits, close_radius=RADIUS.get(kw.get("close_r2", 0), 0), fill_holes=kw.get("fill_holes", True),
                                         open_radius=RADIUS.get(kw.get("open_r2", 0), 0), return_counts=True)
        assert torch.equal(out.cpu(), torch.from_numpy(ref)) and torch.equal(counts.cpu(), torch.from_numpy(refc)), kw
    nchw = torch.from_numpy(x).to(cuda)                  # NCHW storage: the function makes the NHWC copy itself
    assert torch.equal(mgunet.clean_masks(nchw).cpu(), torch.from_numpy(K.clean(cmap, C)[0]))


def test_two_dimensional_map_is_a_batch_of_one(cuda):
    m = blob_map((1, 37, 130), 3, 4)[0]
    out = mgunet.clean_masks(torch.from_numpy(np.array(m)).to(cuda), 3, close_radius=1)
    assert tuple(out.shape) == (1, 37, 130) and torch.equal(out.cpu(), torch.from_numpy(K.clean(m[None], 3, 1)[0]))


def test_structure_across_word_tile_and_labelling_seams(cuda):
    """a thin two-class structure straddling x = 63/64, x = 127/128 and y = 31/32: closing bridges cracks that lie on the seams, the
    opening removes spurs that cross them, and a hole spans four 32 x 32 labelling tiles"""
    m = np.zeros((1, 70, 200), np.int64)
    m[0, 20:45, 50:140] = 1
    m[0, :, 63] = 0
    m[0, :, 64] = 0                                      # a two-pixel crack on the word seam
    m[0, 31, :] = 0                                      # a crack on the tile-row seam
    m[0, 32, 127:129] = 0
    m[0, 26:38, 90:100] = 0                              # a hole over x = 96, y = 32: four labelling tiles
    m[0, 5:20, 63] = 2                                   # spurs on the seams
    m[0, 5:20, 128] = 2
    m[0, 50:52, 120:136] = 2
    m[0, 60:70, 60:68] = 2                               # touches the bottom border across the word seam
    for r2 in R2S:
        check(m, cuda, 3, close_r2=r2, open_r2=r2)
    check(m, cuda, 3)
    check(m, cuda, 3, close_r2=1, fill_holes=False)


def fill_scene():
    m = np.zeros((2, 40, 70), np.int64)
    a = m[0]
    a[2:30, 2:30] = 1
    a[10:20, 10:20] = 0                                  # a hole of 100 pixels ...
    a[14:16, 14:16] = 2                                  # ... with an island of another class: two classes border it, it stays
    a[2:30, 34:50], a[2:30, 50:66] = 1, 2
    a[10:14, 48:52] = 0                                  # a pocket between classes 1 and 2
    a[33:40, 5:15] = 2
    a[36:40, 8:11] = 0                                   # a notch touching the bottom border
    a[34, 20:30], a[36, 20:30], a[35, 20], a[35, 29] = 1, 1, 1, 1   # a one-pixel-high hole of 8
    b = m[1]
    b[5:35, 5:65] = 2
    b[10:20, 10:20] = 0
    b[14:16, 14:16] = 2                                  # an island of the hole's own class: the ring fills, the island stays
    b[25:28, 30:33] = 0                                  # 9 pixels
    b[25:27, 40:45] = 0                                  # 10 pixels
    return m


def test_fill_rules(cuda):
    m = fill_scene()
    out, counts = check(m, cuda, 3)
    assert counts[:, 1].tolist() == [8, 96 + 9 + 10]
    assert (out[0, 10:20, 10:20] == torch.from_numpy(m[0, 10:20, 10:20])).all() and (out[0, 10:14, 48:52] == 0).all()
    _, c9 = check(m, cuda, 3, max_hole_area=9)           # exactly met: the hole of 9 fills, the hole of 10 does not
    assert c9[:, 1].tolist() == [8, 9]
    _, c8 = check(m, cuda, 3, max_hole_area=8)           # exceeded by one
    assert c8[:, 1].tolist() == [8, 0]
    chain = K.chain_scene()[None]
    out, counts = check(chain, cuda, 2)
    assert out[0, 1, 1] == 0 and out[0, 2, 2] == 1 and out[0, 3, 3] == 1 and counts[0].tolist() == [0, 2, 0]


def test_images_do_not_leak(cuda):
    """an object on the bottom rows of image 0, background on the top rows of image 1 (and the reverse): a disc that read across the
    image boundary would erode, close or fill differently"""
    m = np.zeros((3, 33, 66), np.int64)
    m[0, 25:33, 10:50] = 1
    m[0, 29:33, 30] = 0                                  # a crack and a notch on the last rows
    m[1, 0:6, 10:50] = 2
    m[1, 28:33, :] = 1
    m[2, 0, :] = 0
    m[2, 1:5, 20:40] = 1
    for r2 in (1, 4, 9, 64):
        check(m, cuda, 3, close_r2=r2, open_r2=r2)
    for b in range(3):                                   # every image alone gives the same
        alone = run(m[b:b + 1], cuda, 3, close_radius=2, open_radius=2)[0]
        assert torch.equal(alone[0], run(m, cuda, 3, close_radius=2, open_radius=2)[0][b])


def test_repeatable_and_single_stages_idempotent(cuda):
    m = blob_map((2, 61, 131), 3, 7)
    a = run(m, cuda, 3, close_radius=2, open_radius=2)
    b = run(m, cuda, 3, close_radius=2, open_radius=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    filled, _ = run(m, cuda, 3)
    again, counts = run(filled, cuda, 3)
    assert torch.equal(again, filled) and not counts.any()
    for r in (1, 2, 3):
        opened, _ = run(m, cuda, 3, fill_holes=False, open_radius=r)
        again, counts = run(opened, cuda, 3, fill_holes=False, open_radius=r)
        assert torch.equal(again, opened) and not counts.any()


def test_pin_holes_end_to_end(cuda):
    for holes, expected in K.PIN_HOLES:
        m = torch.from_numpy(K.pin_hole_scene(holes))[None].to(cuda)
        assert mgunet.split_objects(m).counts.tolist() == [expected], holes
        assert mgunet.split_objects(mgunet.clean_masks(m, 2)).counts.tolist() == [1], holes


# ---- the evaluators' clean= option ------------------------------------------------------------------------------------------------
def onehot_logits(cmap, C, dev, seed=0):
    """(B, C, H, W) view of NHWC logits whose first maximal class is cmap"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 1, tuple(cmap.shape) + (C,), generator=g).float()
    x.scatter_(-1, cmap.unsqueeze(-1), 1.0)
    return x.to(dev).permute(0, 3, 1, 2)


def evaluator_batches(dev):
    """two batches of two images: discs with pin holes, a cracked disc, a spur, against their clean ground truth"""
    gt = np.zeros((2, 2, 64, 96), np.int64)
    pr = np.zeros_like(gt)
    for k, (holes, _) in enumerate(K.PIN_HOLES[2:]):
        d = K.pin_hole_scene(holes)
        gt[k // 2, k % 2, :, :64] = K.pin_hole_scene(())
        pr[k // 2, k % 2, :, :64] = d
    for b in range(2):
        gt[b, :, 20:50, 70:90], pr[b, :, 20:50, 70:90] = 2, 2
        pr[b, :, 34, 70:90] = 0                          # a crack through the class-2 box
        pr[b, :, 5, 66:96] = 2                           # a spur
    gt[1, 1, 0:3, 0:4] = -100
    return [(onehot_logits(torch.from_numpy(pr[b]), 3, dev, b), torch.from_numpy(gt[b]).to(dev)) for b in range(2)]


CLEAN = {"close_radius": 1, "fill_holes": True, "max_hole_area": 0, "open_radius": 1}
SPLIT = {"min_distance": 5, "min_radius": 3}


def sides(logits, masks, C, clean, split, min_area):
    """the GT and the predicted ObjectTable by the public functions"""
    valid = torch.where((masks >= 0) & (masks < C), masks, torch.zeros_like(masks))
    pred = logits if clean is None else mgunet.clean_masks(logits, **clean)
    tg, tp = mgunet.connected_components(valid), mgunet.connected_components(pred, min_area=min_area)
    if split is not None:
        tg, tp = mgunet.split_objects(tg, **split), mgunet.split_objects(tp, **split)
    return tg, tp


def same_dict(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k], np.float64).view(np.uint64), np.asarray(b[k], np.float64).view(np.uint64)), (k, a[k], b[k])


@pytest.mark.parametrize("split", [None, SPLIT])
def test_yield_evaluator_clean_equals_the_composition(cuda, split):
    batches = evaluator_batches(cuda)
    counts = {}
    for clean in (None, CLEAN):
        ev = mgunet.YieldEvaluator(3, cuda, min_area=2, split=split, clean=clean)
        gt_c, pr_c, gt_l, pr_l = [], [], [], []
        for lg, m in batches:
            ev.update(lg, m)
            tg, tp = sides(lg, m, 3, clean, split, 2)
            gt_c += tg.counts.tolist()
            pr_c += tp.counts.tolist()
            gt_l += tg.to_dicts()
            pr_l += tp.to_dicts()
        res = ev.compute()
        assert list(res) == list(YKEYS)
        same_dict(res, mgunet.yield_estimation_metrics(gt_c, pr_c, gt_l, pr_l))
        counts[clean is None] = res["total_pred_count_sum"]
        if clean is None:                                # the option's default is today's evaluator
            plain = mgunet.YieldEvaluator(3, cuda, min_area=2, split=split)
            for lg, m in batches:
                plain.update(lg, m)
            same_dict(res, plain.compute())
    if split is None:
        assert counts[False] == 8 and counts[True] == 16   # cleaned: one fruit and one box per image


@pytest.mark.parametrize("split", [None, SPLIT])
def test_instance_evaluator_clean_equals_the_composition(cuda, split):
    batches = evaluator_batches(cuda)
    th = (0.5, 0.75)
    for clean in (None, CLEAN):
        ev = mgunet.InstanceEvaluator(3, cuda, thresholds=th, split=split, clean=clean)
        cls, score, tps, pq = [], [], [], np.zeros((3, 4), np.int64)
        for lg, m in batches:
            ev.update(lg, m)
            tg, tp = sides(lg, m, 3, clean, split, 0)
            probs = torch.softmax(lg.permute(0, 2, 3, 1), -1).permute(0, 3, 1, 2)
            sc = mgunet.object_scores(tp, probs)
            ov = mgunet.object_overlaps(tg, tp).check()
            mg, _, _ = mgunet.match_masks(ov, tg, tp, thresholds=th, scores=sc)
            pq += mgunet.panoptic_totals(ov, tg, tp, 3).cpu().numpy()
            cls.append(tp.class_id.cpu().numpy()), score.append(sc.cpu().numpy()), tps.append((mg >= 0).cpu().numpy().reshape(len(th), -1))
        ref = mgunet.instance_metrics(np.concatenate(cls), np.concatenate(score), np.concatenate(tps, 1), pq[:, 0] + pq[:, 2], pq, th)
        res = ev.compute()
        same_dict(res, ref)
        if clean is None:
            plain = mgunet.InstanceEvaluator(3, cuda, thresholds=th, split=split)
            for lg, m in batches:
                plain.update(lg, m)
            same_dict(res, plain.compute())
        elif split is None:
            assert res["total_pred_count_sum"] == 8 and res["PQ"] > 0.9   # every fruit and box found, nearly pixel for pixel


def test_evaluate_functions_pass_clean_on(cuda):
    cfg = (3, 2, 8, 2)
    model = mgunet.UNet(*cfg)
    model.load_state_dict(O.make_unet_params(*cfg, seed=9))
    model = model.to(cuda).eval()
    g = torch.Generator().manual_seed(5)
    masks = torch.from_numpy(K.pin_hole_scene(()))
    loader = [(torch.randn((b, 3, 64, 64), generator=g), masks[None].repeat(b, 1, 1)) for b in (2, 1)]
    clean = {"close_radius": 1.5, "open_radius": 1}
    evs = mgunet.YieldEvaluator(2, cuda, clean=clean), mgunet.InstanceEvaluator(2, cuda, clean=clean)
    with torch.no_grad():
        for x, y in loader:
            lg = model(x.to(cuda))[0]
            for ev in evs:
                ev.update(lg, y.to(cuda))
    same_dict(mgunet.evaluate_yield(model, loader, clean=clean), evs[0].compute())
    same_dict(mgunet.evaluate_instances(model, loader, clean=clean), evs[1].compute())


def test_bad_arguments_raise(cuda):
    m = torch.zeros((1, 8, 8), dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError):
        mgunet.clean_masks(m, 3, close_radius=8.1)       # r2 = 65
    with pytest.raises(ValueError):
        mgunet.clean_masks(m, 3, open_radius=9)
    with pytest.raises(ValueError):
        mgunet.clean_masks(m)                            # a class map needs num_classes
    with pytest.raises(ValueError):
        mgunet.clean_masks(m, 33)
    with pytest.raises(ValueError):
        mgunet.clean_masks(m, 1)
    with pytest.raises(ValueError):
        mgunet.YieldEvaluator(3, cuda, clean={"radius": 2})
    with pytest.raises(ValueError):
        mgunet.InstanceEvaluator(3, cuda, clean={"close_radius": 2, "connectivity": 1})
    with pytest.raises(ValueError):
        mgunet.YieldEvaluator(3, cuda, clean={"open_radius": 9})
    out = torch.empty((1, 8, 8), dtype=torch.int64, device=cuda)
    for args in ((m, 0, 1, 8, 8, 0, 3, 65, 1, 0, 0, out, None), (m, 0, 1, 8, 8, 0, 3, 0, 1, 0, -1, out, None),
                 (m, 0, 1, 8, 8, 0, 40, 0, 1, 0, 0, out, None), (m, 0, 1, 8, 8, 0, 3, 1, 1, 0, 1, m, None),
                 (m, 0, 1, 8, 8, 0, 3, 1, 1, 0, 1, None, None), (m, 2, 1, 8, 8, 0, 3, 1, 1, 0, 1, out, None)):
        with pytest.raises(ValueError):                  # the C entry point: r2, num_classes, aliasing, null pointer, src_kind
            mgunet._lib.call("mgu_clean_masks", cuda, *args)
    empty, counts = mgunet.clean_masks(torch.zeros((0, 4, 4), dtype=torch.int64, device=cuda), 3, return_counts=True)
    assert tuple(empty.shape) == (0, 4, 4) and tuple(counts.shape) == (0, 3)
