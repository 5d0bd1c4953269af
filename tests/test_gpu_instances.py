"""Instance evaluation on the MI355X (csrc/instances.hip, mgunet/instances.py) against tests/instances_oracle.py, bit for bit: the
overlap table (pair_ptr, pair_gt, pair_inter, status), the mask matching (match_gt, match_iou as uint64 views, totals), the panoptic
words; InstanceEvaluator / evaluate_instances against instance_metrics fed from the oracle; YieldEvaluator unchanged."""
import numpy as np
import pytest
import torch

import instances_oracle as IO
import mgunet
import mgunet_oracle as O
import objects_oracle as OO
from mgunet import _lib

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, -7


def run_device(dev, gt, pr, gcls, pcls, thresholds=(0.5,), scores=None, num_classes=3, gt_cap=None, pred_cap=None, pair_cap=None):
    """The three entry points on label maps gt / pr (B, H, W) with per-object classes; capacities default to the object counts and to
    B*H*W pairs.  Every output array carries a guard region behind it, filled with a sentinel."""
    B, H, W = gt.shape
    goff, poff = IO.offsets_of(gt), IO.offsets_of(pr)
    gcap = int(goff[-1]) if gt_cap is None else gt_cap
    pcap = int(poff[-1]) if pred_cap is None else pred_cap
    kcap = B * H * W if pair_cap is None else pair_cap
    T = len(thresholds)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)  # noqa: E731
    glab, plab = (torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)).to(dev) for m in (gt, pr))
    fit = lambda a, n: np.concatenate([a[:n], np.zeros(max(0, n - len(a)), np.int64)])  # noqa: E731
    gc, ga = i64(fit(gcls, gcap)), i64(fit(IO.areas_of(gt), gcap))
    pc, pa = i64(fit(pcls, pcap)), i64(fit(IO.areas_of(pr), pcap))
    go, po = i64(goff), i64(poff)
    guarded = lambda n, dt=torch.int64: torch.full((n + GUARD,), SENTINEL, device=dev, dtype=dt)  # noqa: E731
    ptr, pgt, pin = guarded(pcap + 1), guarded(kcap), guarded(kcap)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("mgu_object_overlaps", dev, glab, go, gcap, plab, po, pcap, B, H, W, kcap, ptr, pgt, pin, status)
    mg, mi = guarded(T * pcap), guarded(T * pcap, torch.float64)
    totals = torch.zeros((T, 3), device=dev, dtype=torch.int64)
    pq = torch.zeros((num_classes, 4), device=dev, dtype=torch.int64)
    sides = (ptr, pgt, pin, kcap, go, gc, ga, gcap, po, pc, pa, pcap)
    sc = None if scores is None else torch.from_numpy(np.ascontiguousarray(fit(scores, pcap).astype(np.float32))).to(dev)
    _lib.call("mgu_match_masks", dev, B, *sides, sc, torch.tensor(list(thresholds), dtype=torch.float64, device=dev), T, mg, mi, totals)
    _lib.call("mgu_panoptic_totals", dev, B, *sides, num_classes, pq)
    torch.cuda.synchronize()
    out = {"pair_ptr": ptr, "pair_gt": pgt, "pair_inter": pin, "match_gt": mg, "match_iou": mi}
    sizes = {"pair_ptr": pcap + 1, "pair_gt": kcap, "pair_inter": kcap, "match_gt": T * pcap, "match_iou": T * pcap}
    res = {"status": int(status.item()), "totals": totals.cpu().numpy(), "pq": pq.cpu().numpy().view(np.uint64), "pcap": pcap, "T": T}
    for k, v in out.items():
        a = v.cpu().numpy()
        assert np.all(a[sizes[k]:] == SENTINEL), f"{k}: written past its end"
        res[k] = a[:sizes[k]]
    return res


def check(dev, gt, pr, gcls, pcls, thresholds=(0.5,), scores=None, num_classes=3, gt_cap=None, pred_cap=None, pair_cap=None):
    """Device against oracle, bitwise; returns both."""
    got = run_device(dev, gt, pr, gcls, pcls, thresholds, scores, num_classes, gt_cap, pred_cap, pair_cap)
    ov = IO.overlaps(gt, pr, gt_cap, pred_cap, got["pair_gt"].size)
    assert got["status"] == ov["status"]
    assert np.array_equal(got["pair_ptr"], ov["pair_ptr"])
    k = ov["pair_gt"].size
    assert np.array_equal(got["pair_gt"][:k], ov["pair_gt"]) and np.array_equal(got["pair_inter"][:k], ov["pair_inter"])
    assert np.all(got["pair_gt"][k:] == SENTINEL) and np.all(got["pair_inter"][k:] == SENTINEL)     # only the pairs present are written
    if ov["status"] & 1:
        return got, ov
    mg, mi, totals = IO.match(gt, pr, gcls, pcls, list(thresholds), scores, gt_cap, pred_cap)
    words, _ = IO.panoptic(gt, pr, gcls, pcls, num_classes, gt_cap, pred_cap)
    T, pcap = got["T"], got["pcap"]
    dmg, dmi = got["match_gt"].reshape(T, pcap), got["match_iou"].reshape(T, pcap)
    n = min(pcap, mg.shape[1])
    goff, poff = IO.offsets_of(gt), IO.offsets_of(pr)
    gcap = int(goff[-1]) if gt_cap is None else gt_cap
    written = np.zeros(pcap, bool)
    for b in range(gt.shape[0]):
        if goff[b + 1] <= gcap and poff[b + 1] <= pcap:                      # an image that was not skipped
            written[poff[b]:poff[b + 1]] = True
    assert np.array_equal(dmg[:, :n][:, written[:n]], mg[:, :n][:, written[:n]])
    assert np.array_equal(dmi[:, :n][:, written[:n]].view(np.uint64), mi[:, :n][:, written[:n]].view(np.uint64))
    assert np.all(dmg[:, ~written] == SENTINEL)                                                       # only rows of objects present
    assert np.array_equal(got["totals"], totals)
    assert np.array_equal(got["pq"], words)
    got.update(o_match_gt=mg, o_match_iou=mi, o_words=words)
    return got, ov


def labelled(cmaps, connectivity=2):
    """(labels int32 (B, H, W), classes (N,)) of class maps through the numpy labelling oracle."""
    labels = np.stack([OO.label(m, connectivity) for m in cmaps])
    return labels, IO.classes_of(labels, cmaps)


def designed_batch():
    """The batch of test_gpu_yield.py.  Image 0: IoU exactly 1/2 (GT [0,0,4,4], prediction [0,0,4,2]); image 1: a prediction at the
    same IoU (1/4) with two GT objects, the first must win; class 2 objects that overlap class 1 objects; image 2: no objects."""
    H, W = 40, 48
    gt = torch.zeros((3, H, W), dtype=torch.int64)
    pr = torch.zeros((3, H, W), dtype=torch.int64)
    gt[0, 0:4, 0:4] = 1
    pr[0, 0:2, 0:4] = 1
    gt[0, 20:30, 20:30] = 2
    pr[0, 22:30, 20:30] = 1                                                 # right place, wrong class
    pr[0, 31:35, 20:30] = 2
    gt[1, 10:14, 0:4] = 1
    gt[1, 10:14, 6:10] = 1
    pr[1, 10:14, 2:8] = 1
    gt[1, 30:34, 30:34] = 2
    pr[1, 30:34, 30:36] = 2
    return gt, pr


def test_designed_batch(cuda):
    gt_c, pr_c = (m.numpy() for m in designed_batch())
    (gt, gcls), (pr, pcls) = labelled(gt_c), labelled(pr_c)
    got, ov = check(cuda, gt, pr, gcls, pcls, thresholds=(0.5, 0.25, 0.5000001, 0.0))
    mg, mi = got["match_gt"].reshape(4, -1), got["match_iou"].reshape(4, -1)
    # prediction 0 of image 0 has IoU exactly 1/2 with GT 0: >= 0.5 matches, the strict panoptic test and 0.5000001 do not
    assert mi[0, 0] == 0.5 and mg[0, 0] == 0 and mg[2, 0] == -1
    assert mg[0, 1] == -1 and mg[3, 1] == -1                                 # right place, wrong class: never, even at threshold 0
    p = int(IO.offsets_of(pr)[1])                                            # image 1, first prediction: IoU 1/4 with two GT objects
    assert mg[1, p] == int(IO.offsets_of(gt)[1]) and mi[1, p] == 0.25 and mg[0, p] == -1
    assert got["pq"][1].tolist()[:3] == [0, 3, 3] and got["pq"][2].tolist()[:3] == [1, 1, 1]
    assert got["pq"][2, 3] == round(16 / 24 * 2 ** 32)
    assert ov["pair_ptr"][-1] == 5


def test_full_image_object_both_sides(cuda):
    ones = np.ones((2, 64, 64), np.int32)
    got, _ = check(cuda, ones, ones, np.array([1, 1]), np.array([1, 1]))
    assert got["pair_ptr"].tolist() == [0, 1, 2] and got["pair_inter"][:2].tolist() == [4096, 4096] and got["pair_gt"][:2].tolist() == [0, 1]
    assert got["pq"][1].tolist() == [2, 0, 0, 2 << 32]


def test_every_pixel_its_own_object(cuda):
    """16 x 16 checkerboards labelled with connectivity 1: 256 objects a side, the most pairs a map can have; pair_capacity = the
    pixel count holds them all, half of it sets status bit 1 and writes nothing past the arrays (run_device checks the guards)."""
    yy, xx = np.mgrid[0:16, 0:16]
    board = torch.from_numpy(((yy + xx) % 2 + 1)[None].astype(np.int64)).to(cuda)
    tg = mgunet.connected_components(board, connectivity=1)
    tp = mgunet.connected_components(3 - board, connectivity=1)
    assert tg.counts.tolist() == [256] and tp.counts.tolist() == [256]
    gt, pr = tg.labels.cpu().numpy(), tp.labels.cpu().numpy()
    gcls, pcls = tg.class_id.cpu().numpy() % 2 + 1, tg.class_id.cpu().numpy() % 2 + 1     # same class per pixel on both sides
    got, ov = check(cuda, gt, pr, gcls, pcls, pair_cap=256)
    assert got["status"] == 0 and ov["pairs"] == 256 and np.array_equal(got["pair_inter"], np.ones(256, np.int64))
    assert int(got["pq"][:, 0].sum()) == 256
    got, ov = check(cuda, gt, pr, gcls, pcls, pair_cap=128)
    assert got["status"] == 1 and got["pair_ptr"][-1] == 256
    table = mgunet.object_overlaps(tg, tp)                                   # the public wrapper on the same tables
    assert np.array_equal(table.check().to_dense(0), np.eye(256, dtype=np.int64))
    with pytest.raises(RuntimeError, match="pair_capacity"):
        mgunet.object_overlaps(tg, tp, pair_capacity=100).check()


def test_run_does_not_cross_the_image_boundary(cuda):
    """B = 3, H*W = 105 (odd, and less than a wave's 256 pixels): label 1 ends image b and starts image b + 1 -- the same local
    label, two different objects."""
    gt = np.zeros((3, 15, 7), np.int32)
    gt[:, 0:2, :] = 1
    gt[:, 13:15, :] = 2
    gt[1, 13:15, :] = 1                                                      # image 1 ends with label 1, image 2 starts with label 1
    gt[1, 0:2, :] = 2
    pr = gt.copy()
    pr[0, 13:15, 3:] = 0
    got, ov = check(cuda, gt, pr, np.ones(6, np.int64), np.ones(6, np.int64))
    assert ov["pairs"] == 6 and got["pair_inter"][:6].tolist() == [14, 6, 14, 14, 14, 14]


def test_runs_on_every_lane_position(cuda):
    """W = 130 (no multiple of the 4 pixels of a lane, nor of 64): rows of horizontal stripes with run lengths 1, 63, 64, 65 and 129
    at shifting offsets, so that runs start and end on every lane position and cross wave boundaries."""
    H, W = 37, 130
    gt = np.zeros((2, H, W), np.int32)
    pr = np.zeros((2, H, W), np.int32)
    lengths = (1, 63, 64, 65, 129)
    for y in range(H):
        n = lengths[y % 5]
        x0 = (7 * y) % (W - n + 1)
        gt[:, y, x0:x0 + n] = 1 + y % 3
        pr[0, y, x0:x0 + n] = 1 + y % 2
        pr[1, y, max(0, x0 - 1):x0 + n - 1] = 1 + (y // 2) % 3
    check(cuda, gt, pr, np.array([1, 2, 1, 1, 2, 1]), np.array([1, 2, 1, 2, 1]), thresholds=(0.5, 0.1))


def blobs(seed, B=4, H=64, W=80, n_obj=32, classes=3):
    """Class maps of random discs (classes 1..classes-1), later ones over earlier ones, and the labelled result."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    cm = np.zeros((B, H, W), np.int64)
    for b in range(B):
        for _ in range(n_obj):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2, 7)
            cm[b][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = rng.randint(1, classes)
    return cm


@pytest.fixture(scope="module")
def blob_case():
    gt_c = blobs(1)
    pr_c = np.roll(gt_c, (1, 2), (1, 2))
    flip = np.random.RandomState(2).rand(*pr_c.shape) < 0.02
    pr_c = np.where(flip, 0, pr_c)
    (gt, gcls), (pr, pcls) = labelled(gt_c), labelled(pr_c)
    rng = np.random.RandomState(3)
    scores = rng.randint(0, 6, pcls.size).astype(np.float32) / 4       # few distinct values: many ties, which fall to the smaller index
    scores[5] = np.nan
    scores[7], scores[8] = 0.0, -0.0
    return gt, gcls, pr, pcls, scores


@pytest.mark.parametrize("T,with_scores", [(10, True), (10, False), (1, True), (16, True)])
def test_random_blobs(cuda, blob_case, T, with_scores):
    gt, gcls, pr, pcls, scores = blob_case
    assert 15 <= IO.offsets_of(gt)[1] <= 40 and IO.offsets_of(pr)[-1] > 90
    th = np.linspace(0.5, 0.95, 10) if T == 10 else np.linspace(0.05, 0.95, T) if T > 1 else np.array([0.3])
    got, _ = check(cuda, gt, pr, gcls, pcls, thresholds=tuple(th), scores=scores if with_scores else None)
    assert got["totals"][-1, 2] <= got["totals"][0, 2] and 0 < got["totals"][0, 2] < got["totals"][0, 0]


def test_scores_change_the_matching(cuda, blob_case):
    """The order matters on this case: with and without scores the matchings differ, each equal to its oracle."""
    gt, gcls, pr, pcls, scores = blob_case
    coarse = np.where(gt > 0, 1, 0).astype(np.int32)                         # one GT object per image: predictions compete for it
    a, _ = check(cuda, coarse, pr, np.ones(4, np.int64), np.ones_like(pcls), thresholds=(0.0,), scores=scores)
    b, _ = check(cuda, coarse, pr, np.ones(4, np.int64), np.ones_like(pcls), thresholds=(0.0,), scores=None)
    assert not np.array_equal(a["match_gt"], b["match_gt"])


def test_object_capacity_skips_an_image(cuda, blob_case):
    gt, gcls, pr, pcls, scores = blob_case
    goff, poff = IO.offsets_of(gt), IO.offsets_of(pr)
    full, _ = check(cuda, gt, pr, gcls, pcls, scores=scores)
    got, ov = check(cuda, gt, pr, gcls, pcls, scores=scores, pred_cap=int(poff[4]) - 1)     # the last image's predictions do not fit
    assert got["status"] == 2 and got["pair_ptr"][-1] == full["pair_ptr"][poff[3]]
    n = int(poff[3])
    assert np.array_equal(got["match_gt"].reshape(1, -1)[:, :n], full["match_gt"].reshape(1, -1)[:, :n])    # the others: unaffected
    got, _ = check(cuda, gt, pr, gcls, pcls, scores=scores, gt_cap=int(goff[4]) - 1)
    assert got["status"] == 2 and got["totals"][0, 0] == goff[3]


def test_bitwise_repeatable(cuda, blob_case):
    gt, gcls, pr, pcls, scores = blob_case
    a = run_device(cuda, gt, pr, gcls, pcls, tuple(np.linspace(0.5, 0.95, 10)), scores)
    b = run_device(cuda, gt, pr, gcls, pcls, tuple(np.linspace(0.5, 0.95, 10)), scores)
    for k in ("pair_ptr", "pair_gt", "pair_inter", "match_gt", "totals", "pq"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["match_iou"].view(np.uint64), b["match_iou"].view(np.uint64))


def test_public_wrappers(cuda):
    """object_overlaps / match_masks / panoptic_totals on ObjectTables equal the raw calls."""
    gt_c = torch.from_numpy(blobs(1)).to(cuda)
    pr_c = torch.roll(gt_c, (1, 2), (1, 2))
    tg, tp = mgunet.connected_components(gt_c), mgunet.connected_components(pr_c)
    gt, pr = tg.labels.cpu().numpy(), tp.labels.cpu().numpy()
    ref = run_device(cuda, gt, pr, tg.class_id.cpu().numpy(), tp.class_id.cpu().numpy(), (0.5, 0.75))
    ov = mgunet.object_overlaps(tg, tp).check()
    mg, mi, totals = mgunet.match_masks(ov, tg, tp, thresholds=(0.5, 0.75))
    assert np.array_equal(ov.pair_ptr.cpu().numpy(), ref["pair_ptr"])
    assert np.array_equal(mg.cpu().numpy().reshape(-1), ref["match_gt"]) and np.array_equal(totals.cpu().numpy(), ref["totals"])
    assert np.array_equal(mi.cpu().numpy().reshape(-1).view(np.uint64), ref["match_iou"].view(np.uint64))
    assert np.array_equal(mgunet.panoptic_totals(ov, tg, tp, 3).cpu().numpy().view(np.uint64), ref["pq"])
    assert np.array_equal(ov.to_dense(1), IO.dense(gt, pr, 1))


# ---- InstanceEvaluator -----------------------------------------------------------------------------------------------------------
def onehot_logits(cmap, C, dev, seed=0):
    """(B, C, H, W) view of NHWC logits whose first maximal class is cmap (ties broken towards the smaller class, as argmax)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 1, tuple(cmap.shape) + (C,), generator=g).float()
    x.scatter_(-1, cmap.unsqueeze(-1), 1.0)
    return x.to(dev).permute(0, 3, 1, 2)


def oracle_metrics(batches, C, thresholds, split=None, min_area=0):
    """instance_metrics fed from the oracle: objects are the (split) device label maps copied to the host, scores mgunet.object_scores
    of the softmax; overlaps, matching and panoptic words all come from tests/instances_oracle.py."""
    cls, score, tps, words = [], [], [], np.zeros((C, 4), np.uint64)
    gt_per_class = np.zeros(C, np.int64)
    for logits, masks in batches:
        clean = torch.where((masks >= 0) & (masks < C), masks, torch.zeros_like(masks))
        if split is None:
            tg, tp = mgunet.connected_components(clean), mgunet.connected_components(logits, min_area=min_area)
        else:
            tg, tp = mgunet.split_objects(clean, **split), mgunet.split_objects(mgunet.connected_components(logits, min_area=min_area), **split)
        probs = torch.softmax(logits.permute(0, 2, 3, 1), -1).permute(0, 3, 1, 2)     # over the NHWC storage, as the evaluator does
        sc = mgunet.object_scores(tp, probs).cpu().numpy()
        gt, pr = tg.labels.cpu().numpy(), tp.labels.cpu().numpy()
        gcls, pcls = tg.class_id.cpu().numpy(), tp.class_id.cpu().numpy()
        poff = IO.offsets_of(pr)
        for b in range(pr.shape[0]):                                   # the order by score is unambiguous: no ties inside an image
            s = sc[poff[b]:poff[b + 1]]
            assert np.unique(s).size == s.size and not np.isnan(s).any()
        c, s, tp_flags, g, w = IO.records(gt, pr, gcls, pcls, list(thresholds), sc, C)
        cls.append(c), score.append(s), tps.append(tp_flags)
        gt_per_class += g
        words += w
    return mgunet.instance_metrics(np.concatenate(cls), np.concatenate(score), np.concatenate(tps, 1), gt_per_class, words, thresholds)


def same_dict(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k], np.float64).view(np.uint64), np.asarray(b[k], np.float64).view(np.uint64)), (k, a[k], b[k])


def evaluator_batches(dev):
    gt, pr = designed_batch()
    gt2, pr2 = torch.zeros((2, 40, 48), dtype=torch.int64), torch.zeros((2, 40, 48), dtype=torch.int64)
    gt2[0, 5:25, 5:25], pr2[0, 6:25, 5:27] = 1, 1
    gt2[0, 30:38, 10:40], pr2[0, 30:38, 10:22], pr2[0, 30:38, 24:40] = 2, 2, 2       # one GT object, two predictions compete
    gt2[1, 8:30, 8:20], gt2[1, 8:30, 20:32] = 1, 2
    pr2[1, 8:30, 8:19], pr2[1, 8:30, 19:32] = 1, 2
    gt2[1, 0:3, 40:44] = -100
    return [(onehot_logits(pr, 3, dev, 1), gt.to(dev)), (onehot_logits(pr2, 3, dev, 2), gt2.to(dev))]


@pytest.mark.parametrize("split", [None, {"min_distance": 3, "min_radius": 2}])
def test_instance_evaluator_equals_oracle(cuda, split):
    batches = evaluator_batches(cuda)
    ev = mgunet.InstanceEvaluator(3, cuda, split=split)
    for lg, m in batches:
        ev.update(lg, m)
    res = ev.compute()
    ref = oracle_metrics(batches, 3, ev.thresholds, split=split)
    same_dict(res, ref)
    if split is None:
        assert 0 < res["PQ"] < 1 and 0 < res["mAP"] < 1 and res["AP50"] >= res["AP75"] and res["total_gt_count_sum"] == 9
    ev.reset()
    ev.update(*batches[1])
    same_dict(ev.compute(), oracle_metrics(batches[1:], 3, ev.thresholds, split=split))
    empty = mgunet.InstanceEvaluator(3, cuda).compute()
    assert empty["mAP"] == 0.0 and empty["PQ"] == 0.0 and empty["total_pred_count_sum"] == 0


def test_evaluate_instances_small_unet(cuda):
    cfg = (3, 2, 8, 2)
    model = mgunet.UNet(*cfg)
    model.load_state_dict(O.make_unet_params(*cfg, seed=9))
    model = model.to(cuda)
    g = torch.Generator().manual_seed(5)
    loader = [(torch.randn((b, 3, 32, 48), generator=g), torch.randint(0, 2, (b, 32, 48), generator=g)) for b in (2, 1)]
    model.train()
    res = mgunet.evaluate_instances(model, loader, thresholds=(0.5, 0.75))
    assert model.training
    model.eval()
    ev = mgunet.InstanceEvaluator(2, cuda, thresholds=(0.5, 0.75))
    with torch.no_grad():
        for x, y in loader:
            ev.update(model(x.to(cuda))[0], y.to(cuda))
    same_dict(res, ev.compute())
    assert res["total_gt_count_sum"] > 0


# ---- YieldEvaluator is unchanged (the check of test_gpu_yield.py on the designed batch) -------------------------------------------
KEYS = ("count_accuracy_perc", "yield_estimation_error_perc", "object_matching_rate_perc", "occlusion_robustness_perc",
        "total_gt_count_sum", "total_pred_count_sum")


def host_metrics(batches, C, connectivity=2, min_area=0, thresh=0.5, smooth=1e-6):
    gt_c, pr_c, gt_l, pr_l = [], [], [], []
    for logits, masks in batches:
        clean = torch.where((masks >= 0) & (masks < C), masks, torch.zeros_like(masks))
        tg = mgunet.connected_components(clean, connectivity=connectivity)
        tp = mgunet.connected_components(logits, connectivity=connectivity, min_area=min_area)
        gt_c += tg.counts.tolist()
        pr_c += tp.counts.tolist()
        gt_l += tg.to_dicts()
        pr_l += tp.to_dicts()
    return mgunet.yield_estimation_metrics(gt_c, pr_c, gt_l, pr_l, matching_iou_thresh=thresh, smooth=smooth)


@pytest.mark.parametrize("thresh", [0.5, 0.25, 0.5000001, 0.0])
def test_yield_evaluator_unchanged(cuda, thresh):
    gt, pr = designed_batch()
    logits = onehot_logits(pr, 3, cuda)
    ev = mgunet.YieldEvaluator(3, cuda, iou_thresh=thresh)
    ev.update(logits, gt.to(cuda))
    a, b = ev.compute(), host_metrics([(logits, gt.to(cuda))], 3, thresh=thresh)
    assert list(a) == list(KEYS) and list(b) == list(KEYS)
    for k in KEYS:
        assert np.array_equal(np.float64(a[k]).view(np.uint64), np.float64(b[k]).view(np.uint64)), (k, a[k], b[k])
