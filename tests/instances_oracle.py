"""numpy / Python oracle of mgunet's instance evaluation (csrc/instances.hip, mgunet/instances.py), shared by the host and the GPU
tests.  Objects of a batch are given as label maps (B, H, W) -- 0 background, objects 1..n_b per image -- with per-object class and
area arrays in batch-wide row order (image after image), as mgunet.ObjectTable holds them.

  overlaps        np.unique over gt_idx * n_pred + pred_idx of the pixels where both labels are non-zero -> CSR by predicted object
  match           the loop of experiments/metrics.py:215-240 with mask IoU, in confidence order, one pass per threshold
  panoptic        strict-majority matching in exact integers; sum of IoU as a Fraction and as the device's fixed-point word
  average_precision_fraction   the AP integral with Fractions (cross-check of the fp64 one in mgunet.instance_metrics)"""
from fractions import Fraction

import numpy as np


def offsets_of(labels):
    """int64 (B + 1): exclusive prefix of the per-image object counts (= the largest label)."""
    counts = [int(m.max()) if m.size else 0 for m in labels]
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


def areas_of(labels):
    """int64 (N): pixels of every object, batch-wide row order."""
    return np.concatenate([np.bincount(m.reshape(-1), minlength=int(m.max()) + 1)[1:] for m in labels] + [np.zeros(0, np.int64)]).astype(np.int64)


def classes_of(labels, values):
    """int64 (N): values[pixel] of every object's pixels (they all agree), batch-wide row order."""
    out = []
    for m, v in zip(labels, values):
        c = np.zeros(int(m.max()), np.int64)
        c[m[m > 0] - 1] = v[m > 0]
        out.append(c)
    return np.concatenate(out + [np.zeros(0, np.int64)])


def image_pairs(g, p):
    """(gt index, pred index, pixels) of one image, local 0-based indices, sorted by (gt, pred): np.unique of the pixel pairs."""
    both = (g > 0) & (p > 0)
    n_pred = int(p.max()) if p.size else 0
    key, cnt = np.unique((g[both].astype(np.int64) - 1) * max(n_pred, 1) + (p[both].astype(np.int64) - 1), return_counts=True)
    return key // max(n_pred, 1), key % max(n_pred, 1), cnt.astype(np.int64)


def overlaps(gt_labels, pred_labels, gt_capacity=None, pred_capacity=None, pair_capacity=None):
    """dict(pair_ptr (pred_capacity + 1), pair_gt, pair_inter (min(pairs, pair_capacity)), status, pairs) as mgu_object_overlaps
    writes them: an image whose objects pass a capacity contributes nothing (status bit 2); pair_ptr keeps the true prefix sums and
    the entries at places >= pair_capacity are dropped (status bit 1)."""
    goff, poff = offsets_of(gt_labels), offsets_of(pred_labels)
    gcap = int(goff[-1]) if gt_capacity is None else gt_capacity
    pcap = int(poff[-1]) if pred_capacity is None else pred_capacity
    rows = [[] for _ in range(pcap)]
    status = 0
    for b, (g, p) in enumerate(zip(gt_labels, pred_labels)):
        if goff[b + 1] > gcap or poff[b + 1] > pcap:
            status |= 2
            continue
        for gi, pi, c in zip(*image_pairs(g, p)):
            rows[int(poff[b] + pi)].append((int(goff[b] + gi), int(c)))
    for r in rows:
        r.sort()
    ptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    flat = [e for r in rows for e in r]
    cap = len(flat) if pair_capacity is None else pair_capacity
    if len(flat) > cap:
        status |= 1
    flat = flat[:cap]
    return {"pair_ptr": ptr, "pair_gt": np.array([e[0] for e in flat], np.int64), "pair_inter": np.array([e[1] for e in flat], np.int64),
            "status": status, "pairs": int(ptr[-1]), "gt_offsets": goff, "pred_offsets": poff}


def dense(gt_labels, pred_labels, b):
    """int64 (n_gt, n_pred) intersection matrix of image b."""
    g, p = gt_labels[b], pred_labels[b]
    out = np.zeros((int(g.max()) if g.size else 0, int(p.max()) if p.size else 0), np.int64)
    for gi, pi, c in zip(*image_pairs(g, p)):
        out[gi, pi] = c
    return out


def score_order(scores):
    """Indices by descending score; ties (-0 = +0 included) to the smaller index; NaN last."""
    def key(i):
        s = float(scores[i])
        return (1, 0.0, i) if s != s else (0, -s, i)
    return sorted(range(len(scores)), key=key)


def match(gt_labels, pred_labels, gt_class, pred_class, thresholds, scores=None, gt_capacity=None, pred_capacity=None):
    """(match_gt int64 (T, N_pred), match_iou float64 (T, N_pred), totals int64 (T, 3)): the greedy loop of metrics.py:215-240 on mask
    IoU = inter / (area_p + area_g - inter) (Python int / int), every threshold with its own used flags.  Rows of skipped images
    keep -1 / 0."""
    goff, poff = offsets_of(gt_labels), offsets_of(pred_labels)
    garea, parea = areas_of(gt_labels), areas_of(pred_labels)
    gcap = int(goff[-1]) if gt_capacity is None else gt_capacity
    pcap = int(poff[-1]) if pred_capacity is None else pred_capacity
    T = len(thresholds)
    mg = np.full((T, int(poff[-1])), -1, np.int64)
    mi = np.zeros((T, int(poff[-1])), np.float64)
    totals = np.zeros((T, 3), np.int64)
    for b in range(len(gt_labels)):
        if goff[b + 1] > gcap or poff[b + 1] > pcap:
            continue
        g0, G, p0, NP = int(goff[b]), int(goff[b + 1] - goff[b]), int(poff[b]), int(poff[b + 1] - poff[b])
        inter = dense(gt_labels, pred_labels, b)
        order = list(range(NP)) if scores is None else score_order(scores[p0:p0 + NP])
        for t, th in enumerate(thresholds):
            used = [False] * G
            for p in order:
                best, best_j = 0, -1
                for j in range(G):
                    if not used[j] and gt_class[g0 + j] == pred_class[p0 + p]:
                        it = int(inter[j, p])
                        iou = it / (int(parea[p0 + p]) + int(garea[g0 + j]) - it) if it else 0.0
                        if iou > best:
                            best, best_j = iou, j
                if best >= th and best_j != -1:
                    used[best_j] = True
                    mg[t, p0 + p], mi[t, p0 + p] = g0 + best_j, best
                    totals[t, 2] += 1
            totals[t, 0] += G
            totals[t, 1] += NP
    return mg, mi, totals


def panoptic(gt_labels, pred_labels, gt_class, pred_class, num_classes, gt_capacity=None, pred_capacity=None):
    """(words uint64 (C, 4): [TP, FP, FN, sum round_half_even(IoU * 2^32)], exact: list of Fractions, the sum of IoU per class).  A
    pair is a TP when the classes agree and 2 * inter > union, in exact integers; objects of a class outside [0, C) and images whose
    objects pass a capacity are ignored."""
    goff, poff = offsets_of(gt_labels), offsets_of(pred_labels)
    garea, parea = areas_of(gt_labels), areas_of(pred_labels)
    gcap = int(goff[-1]) if gt_capacity is None else gt_capacity
    pcap = int(poff[-1]) if pred_capacity is None else pred_capacity
    words = [[0, 0, 0, 0] for _ in range(num_classes)]
    exact = [Fraction(0)] * num_classes
    for b in range(len(gt_labels)):
        if goff[b + 1] > gcap or poff[b + 1] > pcap:
            continue
        for c in pred_class[poff[b]:poff[b + 1]]:
            if 0 <= c < num_classes:
                words[int(c)][1] += 1
        for c in gt_class[goff[b]:goff[b + 1]]:
            if 0 <= c < num_classes:
                words[int(c)][2] += 1
        inter = dense(gt_labels, pred_labels, b)
        for j, p in zip(*np.nonzero(inter)):
            cg, cp = int(gt_class[goff[b] + j]), int(pred_class[poff[b] + p])
            it = int(inter[j, p])
            union = int(parea[poff[b] + p]) + int(garea[goff[b] + j]) - it
            if cg == cp and 0 <= cp < num_classes and 2 * it > union:
                words[cp][0] += 1
                words[cp][1] -= 1
                words[cp][2] -= 1
                exact[cp] += Fraction(it, union)
                words[cp][3] += round(it / union * 4294967296.0)   # Python's round: half to even, exact on a float
    return np.array(words, np.uint64).reshape(num_classes, 4), exact


def average_precision_fraction(tp_sorted, n_gt):
    """Area under the precision envelope of a ranked list of TP flags, all-point interpolation, as a Fraction."""
    tp = fp = 0
    prec, rec = [], []
    for f in tp_sorted:
        tp, fp = tp + bool(f), fp + (not f)
        prec.append(Fraction(tp, tp + fp))
        rec.append(Fraction(tp, n_gt))
    for i in range(len(prec) - 2, -1, -1):
        prec[i] = max(prec[i], prec[i + 1])
    ap, last = Fraction(0), Fraction(0)
    for p, r in zip(prec, rec):
        ap += (r - last) * p
        last = r
    return ap


def records(gt_labels, pred_labels, gt_class, pred_class, thresholds, scores, num_classes):
    """What mgunet.instance_metrics takes, from the oracle: (pred_class, pred_score, pred_tp (T, N), gt_per_class, pq words)."""
    mg, _, _ = match(gt_labels, pred_labels, gt_class, pred_class, thresholds, scores)
    words, _ = panoptic(gt_labels, pred_labels, gt_class, pred_class, num_classes)
    gt_per_class = np.array([int(np.sum(np.asarray(gt_class) == c)) for c in range(num_classes)], np.int64)
    return np.asarray(pred_class), np.asarray(scores, np.float64), mg >= 0, gt_per_class, words
