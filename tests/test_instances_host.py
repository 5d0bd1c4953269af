"""Host tests of the instance evaluation: the numpy oracle (tests/instances_oracle.py) against brute force, the uniqueness of the
panoptic matching, and mgunet.instance_metrics / mgunet.object_detection_mAP on hand-worked examples.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import instances_oracle as IO
import mgunet

EPS = 2.0 ** -50   # a handful of fp64 roundings on values <= 1


def random_maps(seed, B=2, H=24, W=31, n_obj=7, classes=3):
    """Label maps of random rectangles (later ones overwrite earlier ones; emptied labels are squeezed out) and a class per object."""
    rng = np.random.RandomState(seed)
    labels, cls = [], []
    for _ in range(B):
        m = np.zeros((H, W), np.int32)
        for k in range(1, n_obj + 1):
            y, x = rng.randint(0, H - 3), rng.randint(0, W - 3)
            m[y:y + rng.randint(2, 10), x:x + rng.randint(2, 12)] = k
        keep = np.unique(m[m > 0])
        remap = np.zeros(n_obj + 1, np.int32)
        remap[keep] = np.arange(1, keep.size + 1)
        labels.append(remap[m])
        cls.append(rng.randint(1, classes, keep.size))
    return np.stack(labels), np.concatenate(cls).astype(np.int64)


@pytest.mark.parametrize("seed", range(4))
def test_oracle_overlaps_equal_brute_force(seed):
    gt, _ = random_maps(seed)
    pr, _ = random_maps(100 + seed)
    ov = IO.overlaps(gt, pr)
    goff, poff = IO.offsets_of(gt), IO.offsets_of(pr)
    assert ov["status"] == 0 and ov["pair_ptr"][-1] == ov["pair_gt"].size == ov["pairs"] > 0
    for b in range(gt.shape[0]):
        for p in range(int(poff[b + 1] - poff[b])):
            row = slice(int(ov["pair_ptr"][poff[b] + p]), int(ov["pair_ptr"][poff[b] + p + 1]))
            expect = []
            for g in range(int(goff[b + 1] - goff[b])):
                inter = int(np.sum((gt[b] == g + 1) & (pr[b] == p + 1)))
                if inter:
                    expect.append((int(goff[b]) + g, inter))
            assert list(zip(ov["pair_gt"][row].tolist(), ov["pair_inter"][row].tolist())) == expect
        assert np.array_equal(IO.dense(gt, pr, b).sum(), np.sum((gt[b] > 0) & (pr[b] > 0)))


def test_oracle_overlaps_capacities():
    gt, _ = random_maps(7)
    pr, _ = random_maps(8)
    full = IO.overlaps(gt, pr)
    half = IO.overlaps(gt, pr, pair_capacity=full["pairs"] // 2)
    assert half["status"] == 1 and np.array_equal(half["pair_ptr"], full["pair_ptr"])
    assert np.array_equal(half["pair_gt"], full["pair_gt"][:full["pairs"] // 2])
    poff = IO.offsets_of(pr)
    skipped = IO.overlaps(gt, pr, pred_capacity=int(poff[-1]) - 1)     # the last image passes the capacity
    assert skipped["status"] == 2 and skipped["pairs"] == int(full["pair_ptr"][poff[1]])


@pytest.mark.parametrize("seed", range(6))
def test_panoptic_matching_is_the_greedy_matching_just_above_half(seed):
    """IoU > 1/2 can hold for one partner only, so the order-free panoptic matching equals the greedy one at a threshold just above
    1/2 (IoUs here are quotients of integers below 2^10: none lies in (0.5, 0.5 + 1e-9])."""
    gt, gc = random_maps(seed, n_obj=6, classes=3)
    pr = gt.copy()
    rng = np.random.RandomState(seed)
    pr = np.roll(pr, (seed % 2, 1), (1, 2))               # the same objects, shifted: IoUs on both sides of 1/2
    pc = gc.copy()
    pc[rng.rand(pc.size) < 0.2] = 2
    mg, _, totals = IO.match(gt, pr, gc, pc, [0.5 + 1e-9], scores=rng.rand(pc.size).astype(np.float32))
    words, exact = IO.panoptic(gt, pr, gc, pc, 3)
    assert int(words[:, 0].sum()) == int(totals[0, 2]) == int((mg[0] >= 0).sum()) > 0
    for c in range(3):
        assert int(words[c, 0]) == int(np.sum((mg[0] >= 0) & (pc == c)))
        assert abs(float(exact[c]) - int(words[c, 3]) / 2.0 ** 32) <= int(words[c, 0]) * (2.0 ** -33 + 2.0 ** -50)
    matched_gt = mg[0][mg[0] >= 0]
    assert np.unique(matched_gt).size == matched_gt.size                # a GT object is used at most once


def test_match_tie_rules():
    """Equal IoU with two GT objects: the first wins; equal scores (-0 = +0 too) keep list order; NaN sorts last."""
    gt = np.zeros((1, 8, 12), np.int32)
    pr = np.zeros((1, 8, 12), np.int32)
    gt[0, 0:4, 0:4], gt[0, 0:4, 6:10] = 1, 2
    pr[0, 0:4, 2:8] = 1                       # 8 of 24 pixels in each GT object: IoU 8 / 32 with both
    pr[0, 0:4, 8:10] = 2                      # inside GT 2: IoU 8 / 16
    cls = np.ones(2, np.int64)
    for scores in (None, np.array([1.0, 1.0], np.float32), np.array([0.0, -0.0], np.float32)):
        mg, mi, totals = IO.match(gt, pr, cls, cls, [0.25], scores)
        assert mg[0].tolist() == [0, 1] and mi[0].tolist() == [0.25, 0.5] and totals[0].tolist() == [2, 2, 2]
    mg, _, _ = IO.match(gt, pr, cls, cls, [0.6], None)
    assert mg[0].tolist() == [-1, -1]
    assert IO.score_order(np.array([0.5, np.nan, 0.7, 0.5, -np.inf], np.float32)) == [2, 0, 3, 4, 1]


def pq_row(tp, fp, fn, ious):
    return [tp, fp, fn, sum(round(v * 4294967296.0) for v in ious)]


def test_instance_metrics_hand_worked():
    """One class (id 1 of 2), 2 GT objects, predictions in score order TP, FP, TP: precision 1, 1/2, 2/3 -> envelope 1, 2/3, 2/3;
    recall 1/2, 1/2, 1: AP = 1/2 * 1 + 1/2 * 2/3 = 5/6."""
    tp = np.array([[True, True, False]])                       # list order; the scores rank them 0, 2, 1
    m = mgunet.instance_metrics([1, 1, 1], [0.9, 0.7, 0.8], tp, [0, 2], [[0, 0, 0, 0], pq_row(2, 1, 0, [0.75, 0.625])], thresholds=[0.5])
    assert m["AP50"] == pytest.approx(5 / 6, abs=EPS) and m["mAP"] == m["AP50"] == m["AP_per_threshold"][0]
    assert m["AP75"] == -1.0
    assert float(IO.average_precision_fraction([True, False, True], 2)) == pytest.approx(m["AP50"], abs=EPS)
    assert IO.average_precision_fraction([True, False, True], 2) == Fraction(5, 6)
    assert m["SQ"] == pytest.approx((0.75 + 0.625) / 2, abs=EPS) and m["RQ"] == pytest.approx(2 / 2.5, abs=EPS)
    assert m["PQ"] == pytest.approx(m["SQ"] * m["RQ"], abs=EPS)
    assert np.isnan(m["PQ_per_class"][0]) and m["PQ_per_class"][1] == m["PQ"]
    assert m["mask_matching_rate_perc"] == (2 / (2 + 1e-6)) * 100
    assert m["total_gt_count_sum"] == 2 and m["total_pred_count_sum"] == 3


def test_instance_metrics_stable_ties_and_thresholds():
    """Equal scores keep (image order, object index) order: FP first, then TP -> precision 0, 1/2; AP = 1 * 1/2 with one GT."""
    m = mgunet.instance_metrics([0, 0], [0.5, 0.5], [[False, True], [False, False]], [1], [pq_row(1, 1, 0, [0.6])], thresholds=[0.5, 0.75])
    assert m["AP50"] == 0.5 and m["AP75"] == 0.0 and m["mAP"] == 0.25 and m["AP_per_threshold"] == [0.5, 0.0]
    d = mgunet.instance_metrics([], [], np.zeros((10, 0), bool), [0, 3], np.zeros((2, 4), np.int64))
    assert len(d["AP_per_threshold"]) == 10 and d["mAP"] == 0.0 and d["AP50"] == 0.0 and d["AP75"] == 0.0


def test_instance_metrics_class_without_gt_is_skipped_and_no_predictions_score_zero():
    tp = np.array([[True, False, False]])
    pq = [pq_row(1, 0, 0, [1.0]), pq_row(0, 2, 0, []), pq_row(0, 0, 4, [])]
    m = mgunet.instance_metrics([0, 1, 1], [0.9, 0.8, 0.7], tp, [1, 0, 4], pq, thresholds=[0.5])
    # class 0: AP 1; class 1: predictions but no GT, skipped; class 2: GT but no prediction, AP 0
    assert m["AP50"] == 0.5
    assert m["PQ_per_class"] == [1.0, 0.0, 0.0] and m["PQ"] == pytest.approx(1 / 3, abs=EPS)
    none = mgunet.instance_metrics([], [], np.zeros((1, 0), bool), [0, 0, 0], np.zeros((3, 4), np.int64), thresholds=[0.5])
    assert none["AP50"] == 0.0 and none["PQ"] == 0.0 and none["mask_matching_rate_perc"] == 0.0


def test_instance_metrics_two_classes_average():
    tp = np.array([[True, False, True, True]])
    pq = [pq_row(2, 1, 0, [0.75, 0.875]), pq_row(1, 0, 1, [0.625])]
    m = mgunet.instance_metrics([0, 0, 0, 1], [0.9, 0.8, 0.7, 0.6], tp, [2, 2], pq, thresholds=[0.5])
    assert m["AP50"] == pytest.approx((5 / 6 + 1 / 2) / 2, abs=EPS)           # class 1: one TP of two GT objects, precision 1
    assert m["PQ"] == pytest.approx(((0.8125 * 2 / 2.5) + (0.625 * 1 / 1.5)) / 2, abs=EPS)


def boxes_example():
    """The 5/6 example as boxes: GT A and B; predictions hit A (0.9), miss (0.8), hit B (0.7)."""
    gt = [[{"bbox": [0, 0, 10, 10], "class_id": 0, "used": False}, {"bbox": [20, 0, 30, 10], "class_id": 0, "used": False}]]
    pred = [[{"bbox": [0, 0, 10, 8], "class_id": 0, "confidence": 0.9}, {"bbox": [40, 40, 50, 50], "class_id": 0, "confidence": 0.8},
             {"bbox": [20, 0, 30, 9], "class_id": 0, "confidence": 0.7}]]
    return gt, pred


def test_object_detection_map(capsys):
    gt, pred = boxes_example()
    assert mgunet.object_detection_mAP(gt, pred) == pytest.approx(5 / 6, abs=EPS)
    assert capsys.readouterr().out == "" and gt[0][0]["used"] is False
    # at 0.85 only the IoU 0.9 box counts, ranked third: precision 1/3 at recall 1/2
    assert mgunet.object_detection_mAP(gt, pred, iou_threshold=0.85) == pytest.approx(1 / 6, abs=EPS)
    # a second class with one GT box and no prediction halves the mean; a class without GT is skipped
    gt[0].append({"bbox": [60, 60, 70, 70], "class_id": 1, "used": False})
    assert mgunet.object_detection_mAP(gt, pred, num_classes=2) == pytest.approx(5 / 12, abs=EPS)
    assert mgunet.object_detection_mAP(gt, pred, num_classes=3) == pytest.approx(5 / 12, abs=EPS)
    assert mgunet.object_detection_mAP([[]], [[]]) == 0.0


def test_object_detection_map_uses_a_gt_box_once():
    """Two predictions on one GT box: the more confident one is the TP, the other an FP, whatever the list order."""
    gt = [[{"bbox": [0, 0, 10, 10], "class_id": 0}]]
    pred = [[{"bbox": [0, 0, 10, 9], "class_id": 0, "confidence": 0.6}, {"bbox": [0, 0, 10, 10], "class_id": 0, "confidence": 0.9}]]
    assert mgunet.object_detection_mAP(gt, pred) == 1.0           # TP first: precision 1 at recall 1
    pred[0][1]["confidence"] = 0.5                                 # now the 0.9-IoU box goes first and takes the GT box
    assert mgunet.object_detection_mAP(gt, pred) == 1.0
    pred[0][0]["bbox"] = [0, 0, 10, 4]                             # IoU 0.4: an FP first, then the TP: precision 1/2
    assert mgunet.object_detection_mAP(gt, pred) == 0.5
