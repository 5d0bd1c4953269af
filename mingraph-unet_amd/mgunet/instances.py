"""Instance evaluation on mask overlaps: the intersection of every (GT object, predicted object) pair of two label maps, the
confidence-ordered greedy matching of experiments/metrics.py:215-240 on mask IoU at several thresholds, panoptic quality and average
precision -- what experiments/metrics.py:71-140 (object_detection_mAP) describes in its docstring and replaces by a placeholder.

The overlap table, the matching and the panoptic totals run on the device (csrc/instances.hip) in exact integers and fp64 quotients
of integers: bitwise repeatable, a launch count that does not depend on the objects, no host synchronisation.  InstanceEvaluator
accumulates them across batches; the host only integrates the precision-recall curves (instance_metrics, numpy fp64)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .metrics import _evaluate
from .objects import ObjectTable, _iou, _ObjectEvaluator

DEFAULT_THRESHOLDS = np.linspace(0.5, 0.95, 10)   # COCO's 0.50:0.05:0.95


@dataclass
class OverlapTable:
    """Pixels shared by the objects of two ObjectTables of the same images, CSR by predicted object, all on the device and all
    indices batch-wide (rows of the tables' per-object arrays).  pair_ptr: int64 (pred objects + 1); row p is
    [pair_ptr[p], pair_ptr[p + 1]).  pair_gt: int64 (pair_capacity), the GT index, ascending inside a row.  pair_inter: int64
    (pair_capacity), the number of pixels carrying both labels (>= 1).  status: int32 (1): bit 1 = more distinct pairs than
    pair_capacity (the surplus is dropped), bit 2 = an image's objects pass a table's per-object arrays (it contributes no pairs)."""
    pair_ptr: torch.Tensor
    pair_gt: torch.Tensor
    pair_inter: torch.Tensor
    status: torch.Tensor
    gt_offsets: torch.Tensor
    pred_offsets: torch.Tensor

    @property
    def pair_capacity(self) -> int:
        return self.pair_gt.numel()

    def check(self) -> "OverlapTable":
        """Raise unless the table is complete (synchronises)."""
        st = int(self.status.item())
        if st:
            why = [w for bit, w in ((1, f"more distinct pairs than pair_capacity = {self.pair_capacity}"),
                                    (2, "an image's objects pass the per-object arrays")) if st & bit]
            raise RuntimeError("overlap table incomplete: " + "; ".join(why))
        return self

    def to_dense(self, b: int) -> np.ndarray:
        """int64 (n_gt, n_pred): the intersection matrix of image b, for inspection (host; synchronises)."""
        goff, poff = self.gt_offsets.cpu().numpy(), self.pred_offsets.cpu().numpy()
        ptr = self.pair_ptr.cpu().numpy()
        g0, p0 = int(goff[b]), int(poff[b])
        out = np.zeros((int(goff[b + 1]) - g0, int(poff[b + 1]) - p0), np.int64)
        lo, hi = int(ptr[p0]), min(int(ptr[int(poff[b + 1])]), self.pair_capacity)
        pg, pi = self.pair_gt[lo:hi].cpu().numpy(), self.pair_inter[lo:hi].cpu().numpy()
        for p in range(out.shape[1]):
            r0, r1 = int(ptr[p0 + p]) - lo, min(int(ptr[p0 + p + 1]), hi) - lo
            out[pg[r0:r1] - g0, p] = pi[r0:r1]
        return out


def _overlaps(glab, goff, gcap, plab, poff, pcap, B, H, W, pair_ptr, pair_gt, pair_inter, status):
    _lib.call("mgu_object_overlaps", glab.device, glab, goff, int(gcap), plab, poff, int(pcap), B, H, W, pair_gt.numel(), pair_ptr, pair_gt,
              pair_inter, status)


def _sides(ov, gt_off, gt_cls, gt_area, gcap, pred_off, pred_cls, pred_area, pcap):
    """The arguments mgu_match_masks and mgu_panoptic_totals share, after B."""
    return (ov[0], ov[1], ov[2], ov[1].numel(), gt_off, gt_cls, gt_area, int(gcap), pred_off, pred_cls, pred_area, int(pcap))


def _same_images(gt: ObjectTable, pred: ObjectTable, what: str):
    _lib.require_hip(gt.labels, what)
    if gt.labels.shape != pred.labels.shape or gt.labels.device != pred.labels.device:
        raise ValueError(f"{what}: the tables' labels differ in shape or device ({tuple(gt.labels.shape)}, {tuple(pred.labels.shape)})")
    return gt.labels.shape


def object_overlaps(gt: ObjectTable, pred: ObjectTable, pair_capacity: int = None) -> OverlapTable:
    """The overlap table of two ObjectTables (connected_components / split_objects) of the same images.  pair_capacity: the length
    of the pair arrays; the default B*H*W can never overflow (distinct pairs <= pixels).  No dense n_gt x n_pred table is built; a
    fixed number of launches; no host synchronisation (`check()` synchronises)."""
    B, H, W = _same_images(gt, pred, "object_overlaps")
    dev = gt.labels.device
    cap = B * H * W if pair_capacity is None else int(pair_capacity)
    if cap < 0:
        raise ValueError("pair_capacity must be >= 0")
    n_pred = pred.class_id.numel()
    pair_ptr = torch.empty(n_pred + 1, device=dev, dtype=torch.int64)
    pair_gt = torch.empty(cap, device=dev, dtype=torch.int64)
    pair_inter = torch.empty(cap, device=dev, dtype=torch.int64)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _overlaps(gt.labels, gt.offsets, gt.class_id.numel(), pred.labels, pred.offsets, n_pred, B, H, W, pair_ptr, pair_gt, pair_inter, status)
    return OverlapTable(pair_ptr, pair_gt, pair_inter, status, gt.offsets, pred.offsets)


def _thresholds(thresholds) -> np.ndarray:
    th = DEFAULT_THRESHOLDS.copy() if thresholds is None else np.atleast_1d(np.asarray(thresholds, np.float64))
    if th.ndim != 1 or not 1 <= th.size <= 16:
        raise ValueError("between 1 and 16 IoU thresholds")
    return th


def match_masks(overlaps: OverlapTable, gt: ObjectTable, pred: ObjectTable, thresholds=(0.5,), scores: torch.Tensor = None):
    """The greedy matching of experiments/metrics.py:215-240 on mask IoU, every threshold on its own (COCO's way).  Per image the
    predictions are visited by descending `scores` (float32 per predicted object, e.g. mgunet.object_scores; ties: the smaller
    index; NaN last; None: list order); each takes the unused GT object of its class with the largest IoU = inter / union (ties: the
    smaller index) if that IoU is >= the threshold.  Returns (match_gt int64 (T, n_pred): batch-wide GT index or -1, match_iou
    float64 (T, n_pred): the matched IoU or 0, totals int64 (T, 3): [GT objects, predicted objects, matched])."""
    B = _same_images(gt, pred, "match_masks")[0]
    dev = gt.labels.device
    th = _thresholds(thresholds)
    n_pred = pred.class_id.numel()
    if scores is not None:
        if scores.dtype != torch.float32 or scores.numel() != n_pred or scores.device != dev:
            raise ValueError(f"scores must be float32, one per predicted object ({n_pred}), on {dev}")
        scores = scores.contiguous()
    match_gt = torch.full((th.size, n_pred), -1, device=dev, dtype=torch.int64)
    match_iou = torch.zeros((th.size, n_pred), device=dev, dtype=torch.float64)
    totals = torch.zeros((th.size, 3), device=dev, dtype=torch.int64)
    ov = (overlaps.pair_ptr, overlaps.pair_gt, overlaps.pair_inter)
    _lib.call("mgu_match_masks", dev, B, *_sides(ov, gt.offsets, gt.class_id, gt.area, gt.class_id.numel(), pred.offsets, pred.class_id,
                                                 pred.area, n_pred), scores, torch.from_numpy(th).to(dev), th.size, match_gt, match_iou, totals)
    return match_gt, match_iou, totals


def panoptic_totals(overlaps: OverlapTable, gt: ObjectTable, pred: ObjectTable, num_classes: int) -> torch.Tensor:
    """int64 (num_classes, 4): per class [TP, FP, FN, sum over the TP of round(IoU * 2^32)] of panoptic quality's matching: a pair
    is a true positive when the classes agree and IoU > 1/2 (tested exactly in integers; unique per object, so order-free)."""
    B = _same_images(gt, pred, "panoptic_totals")[0]
    pq = torch.zeros((int(num_classes), 4), device=gt.labels.device, dtype=torch.int64)
    ov = (overlaps.pair_ptr, overlaps.pair_gt, overlaps.pair_inter)
    _lib.call("mgu_panoptic_totals", pq.device, B, *_sides(ov, gt.offsets, gt.class_id, gt.area, gt.class_id.numel(), pred.offsets,
                                                           pred.class_id, pred.area, pred.class_id.numel()), int(num_classes), pq)
    return pq


def _average_precision(tp_sorted: np.ndarray, n_gt: int) -> float:
    """Area under the precision envelope of one ranked list of TP flags (all-point interpolation), fp64."""
    if tp_sorted.size == 0:
        return 0.0
    ctp = np.cumsum(tp_sorted, dtype=np.float64)
    cfp = np.cumsum(~tp_sorted, dtype=np.float64)
    precision, recall = ctp / (ctp + cfp), ctp / np.float64(n_gt)
    envelope = np.maximum.accumulate(precision[::-1])[::-1]          # precision made non-increasing from the right
    return float(np.sum(np.diff(np.concatenate(([0.0], recall))) * envelope))


def _ap_table(pred_class, pred_score, pred_tp, gt_per_class) -> np.ndarray:
    """AP (T, C), NaN for a class without GT.  pred_tp: bool (T, N) in (image order, object index) order."""
    T, C = pred_tp.shape[0], len(gt_per_class)
    ap = np.full((T, C), np.nan)
    order = np.argsort(-pred_score, kind="stable")                   # descending score, ties in list order, NaN last
    cls_sorted = pred_class[order]
    for c in range(C):
        if gt_per_class[c] <= 0:
            continue
        sel = order[cls_sorted == c]
        for t in range(T):
            ap[t, c] = _average_precision(pred_tp[t, sel], int(gt_per_class[c]))
    return ap


def _class_mean(v: np.ndarray) -> float:
    ok = ~np.isnan(v)
    return float(np.mean(v[ok])) if ok.any() else 0.0


def instance_metrics(pred_class, pred_score, pred_tp, gt_per_class, pq_totals, thresholds=None, smooth: float = 1e-6) -> dict:
    """Instance metrics of a whole test set from its gathered records, host numpy in fp64.

    pred_class (N,), pred_score (N,), pred_tp bool (T, N): every predicted object's class, confidence and, per IoU threshold, whether
    the greedy matching (match_masks) gave it a GT object, in (image order, object index) order.  gt_per_class (C,): GT objects per
    class.  pq_totals int (C, 4): [TP, FP, FN, sum of round(IoU * 2^32)] per class (panoptic_totals).  thresholds: the T IoU
    thresholds of pred_tp's rows, default np.linspace(0.5, 0.95, 10).

    Average precision of a class at a threshold: take the predictions of that class over the WHOLE set, sort them by descending
    score (stable: ties keep their order), form the cumulative TP and FP counts, precision = TP / (TP + FP) and recall =
    TP / (GT objects of the class); make the precision non-increasing from the right (the envelope) and sum it over the recall
    increments (all-point interpolation, no 101-point sampling).  A class with no GT object is skipped; a class with GT and no
    prediction scores 0.  AP_per_threshold[t] is the mean over the classes, mAP the mean over the thresholds given, AP50 / AP75 the
    entries of the thresholds equal to 0.5 / 0.75 (-1.0 when not among them).

    Panoptic quality per class: SQ = sum IoU / TP (0 without a TP), RQ = TP / (TP + FP / 2 + FN / 2), PQ = SQ * RQ; PQ, SQ and RQ
    are the means over the classes that have a GT object or a prediction (PQ_per_class holds NaN for the others).
    mask_matching_rate_perc is object_matching_rate_perc's formula, matched / (GT objects + smooth) * 100, with the mask matching at
    the first threshold."""
    th = _thresholds(thresholds)
    pred_class = np.asarray(pred_class, np.int64).reshape(-1)
    pred_score = np.asarray(pred_score, np.float64).reshape(-1)
    pred_tp = np.asarray(pred_tp, bool).reshape(th.size, pred_class.size)
    gt_per_class = np.asarray(gt_per_class, np.int64).reshape(-1)
    pq_totals = np.asarray(pq_totals).astype(np.uint64).reshape(-1, 4)
    if not pred_class.size == pred_score.size == pred_tp.shape[1]:
        raise ValueError("pred_class, pred_score and pred_tp disagree on the number of predictions")
    if pq_totals.shape[0] != gt_per_class.size:
        raise ValueError("pq_totals and gt_per_class disagree on the number of classes")
    ap = _ap_table(pred_class, pred_score, pred_tp, gt_per_class)
    ap_t = np.array([_class_mean(ap[t]) for t in range(th.size)])

    def at(v):
        hit = np.nonzero(np.isclose(th, v, rtol=0, atol=1e-9))[0]
        return float(ap_t[hit[0]]) if hit.size else -1.0

    tp, fp, fn = (pq_totals[:, k].astype(np.float64) for k in range(3))
    siou = pq_totals[:, 3].astype(np.float64) / 4294967296.0
    seen = (tp + fp + fn) > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.where(tp > 0, siou / tp, 0.0)
        rq = np.where(seen, tp / (tp + fp / 2 + fn / 2), np.nan)
    sq = np.where(seen, sq, np.nan)
    pq = sq * rq
    matched = int(pred_tp[0].sum()) if pred_tp.shape[1] else 0
    return {"PQ": _class_mean(pq), "SQ": _class_mean(sq), "RQ": _class_mean(rq), "PQ_per_class": pq.tolist(),
            "AP_per_threshold": ap_t.tolist(), "AP50": at(0.5), "AP75": at(0.75), "mAP": float(np.mean(ap_t)),
            "mask_matching_rate_perc": (matched / (int(gt_per_class.sum()) + smooth)) * 100,
            "total_gt_count_sum": int(gt_per_class.sum()), "total_pred_count_sum": int(pred_class.size)}


def object_detection_mAP(gt_boxes_list, pred_boxes_list, iou_threshold=0.5, num_classes=1) -> float:
    """experiments/metrics.py:71-140 object_detection_mAP with the steps its docstring lists carried out: same arguments -- per image
    a list of GT dicts {'bbox': [xmin, ymin, xmax, ymax], 'class_id': int} (a 'used' key is ignored and not modified) and of
    predicted dicts {'bbox', 'class_id', 'confidence': float} -- the reference's greedy box-IoU matching per image in descending
    confidence, then per class the average precision defined in instance_metrics over the whole set, averaged over the classes
    0..num_classes-1 that have a GT box.  Host Python.  The reference returns (precision + recall) / 2 of one pooled count, which
    its own comments call a dummy value, so the two cannot be compared."""
    cls, conf, tps = [], [], []
    n_gt = np.zeros(int(num_classes), np.int64)
    for gts, preds in zip(gt_boxes_list, pred_boxes_list):
        used = [False] * len(gts)
        for g in gts:
            if 0 <= g["class_id"] < num_classes:
                n_gt[g["class_id"]] += 1
        hits = {}
        for k, p in sorted(enumerate(preds), key=lambda kp: kp[1]["confidence"], reverse=True):
            best, best_j = 0, -1
            for j, g in enumerate(gts):
                if g["class_id"] == p["class_id"] and not used[j]:
                    iou = _iou(p["bbox"], g["bbox"])
                    if iou > best:
                        best, best_j = iou, j
            hits[k] = bool(best >= iou_threshold and best_j != -1)
            if hits[k]:
                used[best_j] = True
        for k, p in enumerate(preds):
            cls.append(p["class_id"]), conf.append(p["confidence"]), tps.append(hits[k])
    ap = _ap_table(np.array(cls, np.int64), np.array(conf, np.float64), np.array(tps, bool).reshape(1, len(tps)), n_gt)
    return _class_mean(ap[0])


class InstanceEvaluator(_ObjectEvaluator):
    """Device-side instance evaluation over a test set, in the shape of YieldEvaluator.  update(logits, masks) labels the predicted
    objects (argmax fused; min_area applies to them) and the GT objects (connected components of the mask values in
    [1, num_classes); with `split` both are cut apart as YieldEvaluator does), takes per-object classes and areas, scores every
    prediction by the mean softmax probability of its class over its pixels (mgunet.object_scores), builds the overlap table, matches
    at every threshold in score order and accumulates the panoptic totals; the per-prediction records (class, score, one TP bit per
    threshold) are kept on the device and the host is never blocked.  Every buffer is sized once for the worst case (every pixel its
    own object), the records included: 12 bytes per pixel of every batch until reset().  compute() synchronises once and returns
    instance_metrics' dictionary; it raises if the overlap table's status is non-zero.  clean: as YieldEvaluator's -- the predicted
    class map is cleaned (mgunet.clean_masks) before it is labelled and split; scores still come from the logits."""

    def __init__(self, num_classes: int, device, connectivity: int = 2, min_area: int = 0, thresholds=None, split: dict = None,
                 smooth: float = 1e-6, clean: dict = None):
        super().__init__(num_classes, device, connectivity, min_area, split, clean)
        self.smooth = smooth
        self.thresholds = _thresholds(thresholds)
        T = self.thresholds.size
        self._thr = torch.from_numpy(self.thresholds).to(self.device)
        self._bit = (2 ** torch.arange(T, dtype=torch.int32)).view(T, 1).to(self.device)
        self.reset()

    def reset(self) -> None:
        T = self.thresholds.size
        self.totals = torch.zeros((T, 3), device=self.device, dtype=torch.int64)   # per threshold: GT objects, predictions, matched
        self.pq = torch.zeros((self.num_classes, 4), device=self.device, dtype=torch.int64)
        self.status = torch.zeros(1, device=self.device, dtype=torch.int32)
        self._records = []   # per batch: (predictions present (1,), class (n,), score (n,), TP bits (n,)), rows past the first entry unused

    def _buffers(self, n):
        if n > self._cap:
            mk = lambda shape, dt: torch.empty(shape, device=self.device, dtype=dt)  # noqa: E731
            T = self.thresholds.size
            b = {s: (mk(n, torch.int32), mk(n, torch.int64), mk((n, 4), torch.int32), mk(n, torch.int64)) for s in ("gt", "pred")}
            b["scores"] = mk(n, torch.float32)
            b["pairs"] = (mk(n + 1, torch.int64), mk(n, torch.int64), mk(n, torch.int64))
            b["match"] = (mk((T, n), torch.int64), mk((T, n), torch.float64))
            if self._clean is not None:
                b["clean"] = mk(n, torch.int64)
            self._bufs, self._cap = b, n
        return self._bufs

    def update(self, logits_nchw: torch.Tensor, masks: torch.Tensor) -> None:
        """Add one batch: logits (B, C, H, W) float32 -- the view UNet.forward returns -- and integer masks (B, H, W)."""
        src, masks, B, H, W, C = self._batch(logits_nchw, masks)
        n = B * H * W
        bufs, cap = self._buffers(n), self._cap
        _, offsets = self._label_sides(src, masks, B, H, W, C, bufs)
        (gl, gc, _, ga), (pl, pc, _, pa) = bufs["gt"], bufs["pred"]
        probs = torch.softmax(src, dim=-1)   # NHWC, as mgu_object_scores reads it
        _lib.call("mgu_object_scores", self.device, pl, probs, B, H, W, C, offsets["pred"], cap, pc, pa, bufs["scores"])
        _overlaps(gl, offsets["gt"], cap, pl, offsets["pred"], cap, B, H, W, *bufs["pairs"], self.status)
        mg, mi = bufs["match"]
        sides = _sides(bufs["pairs"], offsets["gt"], gc, ga, cap, offsets["pred"], pc, pa, cap)
        _lib.call("mgu_match_masks", self.device, B, *sides, bufs["scores"], self._thr, self.thresholds.size, mg, mi, self.totals)
        _lib.call("mgu_panoptic_totals", self.device, B, *sides, self.num_classes, self.pq)
        bits = ((mg[:, :n] >= 0).to(torch.int32) * self._bit).sum(0, dtype=torch.int32)   # rows past the objects present: unused
        self._records.append((offsets["pred"][B:].clone(), pc[:n].to(torch.int32), bufs["scores"][:n].clone(), bits))

    def compute(self) -> dict:
        """Synchronise once and return instance_metrics' dictionary over every batch since the last reset()."""
        T = self.thresholds.size
        status = int(self.status.item())
        if status:
            raise RuntimeError(f"InstanceEvaluator: the overlap table reported status {status} (1: pair capacity, 2: object capacity)")
        pq = self.pq.cpu().numpy()
        gt_per_class = pq[:, 0] + pq[:, 2]
        if self._records:
            counts = torch.cat([r[0] for r in self._records]).cpu().tolist()
            cls = torch.cat([r[1][:k] for r, k in zip(self._records, counts)]).cpu().numpy()
            score = torch.cat([r[2][:k] for r, k in zip(self._records, counts)]).cpu().numpy()
            bits = torch.cat([r[3][:k] for r, k in zip(self._records, counts)]).cpu().numpy()
        else:
            cls, score, bits = np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int32)
        tp = ((bits[None, :] >> np.arange(T, dtype=np.int32)[:, None]) & 1).astype(bool)
        return instance_metrics(cls, score, tp, gt_per_class, pq, self.thresholds, self.smooth)


def evaluate_instances(model, loader, num_classes=None, connectivity=2, min_area=0, thresholds=None, split=None, smooth=1e-6,
                       clean=None) -> dict:
    """Instance evaluation over `loader`'s (images, masks) batches: logits = model(images) under torch.no_grad() in eval mode, then
    InstanceEvaluator.  Returns instance_metrics' dictionary; the model's training flag is restored."""
    return _evaluate(model, loader, num_classes, lambda C, dev: InstanceEvaluator(
        C, dev, connectivity=connectivity, min_area=min_area, thresholds=thresholds, split=split, smooth=smooth, clean=clean))
