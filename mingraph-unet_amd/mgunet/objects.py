"""Object counting and yield estimation: the instance step model/unet/shape_loss.py:43-91 leaves commented out
(skimage.measure.label) and experiments/metrics.py:160-253 (yield_estimation_metrics).

Connected components, per-object statistics and the reference's greedy box matching all run on the device (csrc/objects.hip);
YieldEvaluator accumulates per-image counts and matching totals across batches without a host synchronisation, and the host only
turns them into the reference's dictionary with the reference's own arithmetic (bitwise equal results).  object_shapes adds the
per-object shape (csrc/shapes.hip): exact integer moments of the label map, a fitted ellipse and the per-instance term of
EllipticalShapeLoss (model/unet/shape_loss.py:155-180).  split_objects cuts touching objects apart (csrc/split.hip): exact integer
distance transform, one seed per inscribed disc, the power diagram of the discs.  clean_masks tidies the class map before any of
this (csrc/clean.hip): closing, hole filling and opening on bit planes.  There is no scipy or skimage dependency."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._args import batched_map, nhwc_storage
from .metrics import _Evaluator, _evaluate


@dataclass
class ObjectTable:
    """Objects of a batch, all on the device.  labels: int32 (B, H, W), 0 = background, objects 1..n_b per image in raster order of
    their first pixel.  counts: int64 (B).  offsets: int64 (B + 1), object k of image b is row offsets[b] + k - 1 of the per-object
    arrays: class_id int64 (N), area int64 (N), bbox int32 (N, 4) [xmin, ymin, xmax, ymax] with exclusive max edges, sums int64
    (N, 2) [sum x, sum y] (centroid = sums / area)."""
    labels: torch.Tensor
    counts: torch.Tensor
    offsets: torch.Tensor
    class_id: torch.Tensor
    area: torch.Tensor
    bbox: torch.Tensor
    sums: torch.Tensor

    def to_dicts(self, scores=None, shapes=None, runs=None, outlines=None) -> list:
        """The reference's per-image object lists: [[{'bbox': [xmin, ymin, xmax, ymax], 'class_id': int}, ...], ...].  With scores
        (one float per object in row order, e.g. mgunet.object_scores), every dict also carries 'confidence': float, the key
        yield_estimation_metrics sorts predictions by.  With shapes (mgunet.object_shapes of this table), every dict also carries
        'ellipse': {'center': [x, y], 'axes': [a, b], 'angle': radians, 'fill': f} and 'shape_term': float; both are None for an
        object that was not analysed (shapes.status != 0).  With runs (mgunet.encode_masks of this table), every dict also carries
        'segmentation': COCO's compressed RLE {'size': [H, W], 'counts': str}; with outlines (mgunet.object_outlines of this table),
        'segmentation' is COCO's polygon form, a list of flat [x0, y0, x1, y1, ...] outer loops (holes are not expressible in it).  With
        both given, runs wins."""
        off = self.offsets.cpu().tolist()
        bbox, cls = self.bbox.cpu().tolist(), self.class_id.cpu().tolist()
        rows = [{"bbox": bbox[i], "class_id": cls[i]} for i in range(len(cls))]
        if scores is not None:
            conf = scores.cpu().tolist() if isinstance(scores, torch.Tensor) else [float(v) for v in scores]
            if len(conf) != len(cls):
                raise ValueError(f"{len(conf)} scores for {len(cls)} objects")
            for d, v in zip(rows, conf):
                d["confidence"] = v
        if shapes is not None:
            if shapes.status.numel() != len(cls):
                raise ValueError(f"shapes of {shapes.status.numel()} objects for {len(cls)} objects")
            cen, axes, st = shapes.centroid.cpu().tolist(), shapes.axes.cpu().tolist(), shapes.status.cpu().tolist()
            ang, fill, term = shapes.angle.cpu().tolist(), shapes.fill.cpu().tolist(), shapes.term.cpu().tolist()
            for i, d in enumerate(rows):
                ok = st[i] == 0
                d["ellipse"] = {"center": cen[i], "axes": axes[i], "angle": ang[i], "fill": fill[i]} if ok else None
                d["shape_term"] = term[i] if ok else None
        seg = runs if runs is not None else outlines
        if seg is not None:
            flat = [s for per in seg.to_coco() for s in per]
            if len(flat) != len(cls):
                raise ValueError(f"segmentations of {len(flat)} objects for {len(cls)} objects")
            for d, s in zip(rows, flat):
                d["segmentation"] = s
        return [rows[off[b]:off[b + 1]] for b in range(len(off) - 1)]

    def masks(self) -> list:
        """object_masks_list of EllipticalShapeLoss: per image, one bool (H, W) device mask per object, in label order.  Dense: M
        full-image masks and a host synchronisation.  For the loss and the shape of every object use mgunet.object_shapes(table)
        (or EllipticalShapeLoss()(None, objects=table)), which reads the label map once and builds no masks."""
        counts = self.counts.cpu().tolist()
        return [[self.labels[b] == k for k in range(1, n + 1)] for b, n in enumerate(counts)]


def _source(x: torch.Tensor):
    """(src tensor, kind, B, H, W, C): an int64 class map (kind 0) or the NHWC storage of (B, C, H, W) fp32 logits (kind 1)."""
    _lib.require_hip(x, "connected components")
    if x.is_floating_point():
        if x.dim() != 4 or x.dtype != torch.float32:
            raise TypeError("logits must be (B, C, H, W) float32")
        B, C, H, W = x.shape
        return nhwc_storage(x), 1, B, H, W, C
    m = batched_map(x, "a class map")
    B, H, W = m.shape
    return m.to(torch.int64).contiguous(), 0, B, H, W, 0


def _clean_params(close_radius=0, fill_holes=True, max_hole_area=0, open_radius=0):
    """(close_radius_sq, fill_holes, max_hole_area, open_radius_sq) as mgu_clean_masks takes them: floor(radius^2), 0..64 (a hair
    is added before the floor, so that math.sqrt(13) squares to 13 and not to 12)."""
    r2 = []
    for name, r in (("close_radius", close_radius), ("open_radius", open_radius)):
        if not r >= 0:
            raise ValueError(f"{name} must be >= 0")
        r2.append(math.floor(r * r + 1e-9))
        if r2[-1] > 64:
            raise ValueError(f"{name} {r}: the squared radius must stay within 64")
    if max_hole_area < 0:
        raise ValueError("max_hole_area must be >= 0")
    return r2[0], int(bool(fill_holes)), int(max_hole_area), r2[1]


def _clean(src, kind, B, H, W, C, num_classes, params, out, counts=None):
    _lib.call("mgu_clean_masks", src.device, src, kind, B, H, W, C, int(num_classes), *params, out, counts)


def clean_masks(x: torch.Tensor, num_classes: int = None, close_radius: float = 0, fill_holes: bool = True, max_hole_area: int = 0,
                open_radius: float = 0, return_counts: bool = False):
    """The class map of x with gaps closed, holes filled and spurs opened away, on the device: the stage between argmax and
    connected_components / split_objects, whose distance transform a single pin hole inside a fruit breaks.

    x: whatever connected_components takes -- an integer class map (H, W) or (B, H, W), for which num_classes is required, or
    (B, C, H, W) float32 logits (argmax fused; num_classes is C).  Classes 1 .. num_classes - 1 (num_classes <= 32) are foreground;
    every other value is background and comes out as 0.  Returns the int64 (B, H, W) class map; an (H, W) map is a batch of one.

    With D(r) the disc {d : |d|^2 <= floor(r^2)}, r <= 8, three stages in this order, each skipped when its parameter is 0 / False:
    close_radius -- a background pixel p takes the smallest class c whose dilation by D covers p + D (pixels outside the image are
    background; foreground never changes); fill_holes -- a 4-connected background component that touches no image border, has at most
    max_hole_area pixels (when > 0) and whose foreground 4-neighbours all hold one class becomes that class (a pocket between two
    classes stays, an island inside a hole is untouched); open_radius -- a pixel of class c stays iff a pixel q of class c within D
    of it has no image pixel of another value within D of q (pixels outside the image do not erode: an object cut by the frame keeps
    its edge).  Not a per-object convex hull and no grey-level morphology.  Integer and bit arithmetic: bitwise repeatable; a fixed
    number of launches and no host synchronisation.  return_counts: also the int64 (B, 3) pixels [gained by closing, filled, removed
    by opening] per image."""
    params = _clean_params(close_radius, fill_holes, max_hole_area, open_radius)
    src, kind, B, H, W, C = _source(x)
    if kind == 0 and num_classes is None:
        raise ValueError("clean_masks: num_classes is required for a class map")
    ncls = C if kind == 1 else int(num_classes)
    if not 2 <= ncls <= 32:
        raise ValueError(f"clean_masks: num_classes must be in 2..32, got {ncls}")
    out = torch.empty((B, H, W), device=src.device, dtype=torch.int64)
    counts = torch.zeros((B, 3), device=src.device, dtype=torch.int64) if return_counts else None
    if out.numel():   # a batch without pixels has no storage to point at
        _clean(src, kind, B, H, W, C, ncls, params, out, counts)
    return (out, counts) if return_counts else out


def _label(src, kind, B, H, W, C, connectivity, background, num_classes, min_area, labels, counts, offsets):
    _lib.call("mgu_connected_components", src.device, src, kind, B, H, W, C, int(connectivity), int(background), int(num_classes),
              int(min_area), labels, counts, offsets)


def _stats(labels, src, kind, B, H, W, C, offsets, capacity, cls, bbox, area=None, sums=None):
    _lib.call("mgu_object_stats", src.device, labels, src, kind, B, H, W, C, offsets, int(capacity), cls, area, bbox, sums)


def _check_args(connectivity, min_area):
    if connectivity not in (1, 2):
        raise ValueError(f"connectivity must be 1 (4-neighbours) or 2 (8-neighbours), got {connectivity}")
    if min_area < 0:
        raise ValueError("min_area must be >= 0")


def _table(labels, counts, offsets, src, kind, C) -> ObjectTable:
    """The ObjectTable of a labelled batch: per-object arrays sized from offsets[B] (one synchronisation) and filled by _stats."""
    B, H, W = labels.shape
    dev = labels.device
    N = int(offsets[B].item())
    cls = torch.empty(N, device=dev, dtype=torch.int64)
    area = torch.empty(N, device=dev, dtype=torch.int64)
    bbox = torch.empty((N, 4), device=dev, dtype=torch.int32)
    sums = torch.empty((N, 2), device=dev, dtype=torch.int64)
    if N:
        _stats(labels, src, kind, B, H, W, C, offsets, N, cls, bbox, area, sums)
    return ObjectTable(labels, counts, offsets, cls, area, bbox, sums)


def connected_components(x: torch.Tensor, connectivity: int = 2, background: int = 0, min_area: int = 0) -> ObjectTable:
    """skimage.measure.label(x, connectivity, background) per image, plus per-object statistics, on the device.

    x: an integer class map (H, W) or (B, H, W) -- every value other than `background` is foreground, and pixels join when they are
    neighbours holding the same value -- or (B, C, H, W) float32 logits (the NCHW view UNet.forward returns, its NHWC storage read in
    place), whose per-pixel class is the first maximal one (= torch.argmax(x, 1)).  Objects smaller than min_area pixels become
    background.  An (H, W) map is labelled as a batch of one.  Synchronises once, to size the per-object arrays."""
    _check_args(connectivity, min_area)
    src, kind, B, H, W, C = _source(x)
    dev = src.device
    labels = torch.empty((B, H, W), device=dev, dtype=torch.int32)
    counts = torch.empty(B, device=dev, dtype=torch.int64)
    offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    _label(src, kind, B, H, W, C, connectivity, background, 0, min_area, labels, counts, offsets)
    return _table(labels, counts, offsets, src, kind, C)


def distance_transform(labels) -> torch.Tensor:
    """int32 (B, H, W): the exact squared Euclidean distance of every foreground pixel of an integer label map (H, W) or (B, H, W),
    or of an ObjectTable's labels, to the nearest pixel of its image holding another label (background or another object; pixels
    outside the image do not count: scipy.ndimage.distance_transform_edt(labels == k) ** 2 on the pixels of label k).  0 on
    background, 2 ** 30 where the image holds no other label.  H, W <= 16384.  The labels are read as int32: every value of a wider
    map must fit it (connected_components' labels do), or distinct labels may wrap onto each other or onto 0."""
    lab = labels.labels if isinstance(labels, ObjectTable) else labels
    _lib.require_hip(lab, "distance_transform")
    lab = batched_map(lab, "a label map").to(torch.int32).contiguous()
    B, H, W = lab.shape
    d2 = torch.empty((B, H, W), device=lab.device, dtype=torch.int32)
    _lib.call("mgu_distance_transform", lab.device, lab, B, H, W, d2)
    return d2


def _split_params(min_distance, min_radius, min_area):
    """(min_distance, min_radius_sq, min_area) as mgu_split_objects takes them: the radius is squared here."""
    if int(min_distance) != min_distance or not 1 <= min_distance <= 16:
        raise ValueError(f"min_distance must be an integer in 1..16, got {min_distance}")
    if not min_radius > 0:
        raise ValueError("min_radius must be > 0")
    if min_area < 0:
        raise ValueError("min_area must be >= 0")
    return int(min_distance), max(1, math.ceil(min_radius * min_radius)), int(min_area)


def _split(labels, B, H, W, params, out, counts, offsets, d2=None, seeds=None):
    _lib.call("mgu_split_objects", labels.device, labels, B, H, W, *params, out, counts, offsets, d2, seeds)


def split_objects(x, min_distance: int = 5, min_radius: float = 3, connectivity: int = 2, background: int = 0, min_area: int = 0,
                  return_seeds: bool = False):
    """connected_components(x, connectivity, background) with touching objects cut apart, on the device.  x: whatever
    connected_components takes, or an ObjectTable (its labels are split; connectivity and background are not used then).

    Every object gets the exact squared distance transform D2 of its mask.  A pixel is a seed when D2 >= min_radius ** 2 and no pixel
    of its object within Chebyshev distance min_distance (1..16) has a larger D2; seeds whose (min_distance + 1) // 2 neighbourhoods
    touch are one group.  Each pixel goes to the group of the seed s minimising |p - s|^2 - D2(s): the power diagram of the inscribed
    discs, which cuts two overlapping discs along the chord through their intersection points.  An object thinner than min_radius
    stays whole.  Objects under min_area pixels are dropped after the split.  This is not a flooding watershed: a ring of three
    mutually overlapping discs can yield a fourth cell at the enclosed centre peak (raise min_radius), and strongly non-convex blobs
    over-split, as under any prominence-free seed rule.  All integer arithmetic: bitwise repeatable.  Synchronises once, to size the
    per-object arrays.  return_seeds: also return the bool (B, H, W) seed mask."""
    _check_args(connectivity, min_area)
    params = _split_params(min_distance, min_radius, min_area)
    parent = x if isinstance(x, ObjectTable) else None
    if parent is not None:
        _lib.require_hip(parent.labels, "split_objects")
        B, H, W = parent.labels.shape
        comp, dev = parent.labels, parent.labels.device
        src, kind, C = parent.labels.to(torch.int64), 0, 0   # the statistics' "class" of a new object: its parent's label
    else:
        src, kind, B, H, W, C = _source(x)
        dev = src.device
        comp = torch.empty((B, H, W), device=dev, dtype=torch.int32)
        _label(src, kind, B, H, W, C, connectivity, background, 0, 0, comp, torch.empty(B, device=dev, dtype=torch.int64),
               torch.empty(B + 1, device=dev, dtype=torch.int64))
    labels = torch.empty((B, H, W), device=dev, dtype=torch.int32)
    counts = torch.empty(B, device=dev, dtype=torch.int64)
    offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
    seeds = torch.empty((B, H, W), device=dev, dtype=torch.uint8) if return_seeds else None
    _split(comp, B, H, W, params, labels, counts, offsets, None, seeds)
    table = _table(labels, counts, offsets, src, kind, C)
    N = table.class_id.numel()
    if N and parent is not None:   # parent label -> the parent's row -> its class
        image = torch.repeat_interleave(torch.arange(B, device=dev), counts, output_size=N)
        table.class_id = parent.class_id[parent.offsets[image] + table.class_id - 1]
    return (table, seeds.bool()) if return_seeds else table


@dataclass
class ObjectShapes:
    """Per-object shape of an ObjectTable, all on the device, rows in the table's object order.  centroid (N, 2) [x, y] in image
    coordinates; cov (N, 3) [c_xx, c_xy, c_yy], the sample covariance of the pixel coordinates (divisor n - 1); axes (N, 2) [a, b],
    the semi-axes in pixels of the uniformly filled ellipse with that covariance (2 sqrt of its eigenvalues, a >= b); angle (N),
    radians, the major axis from +x towards +y; fill (N) = area / (pi a b); term (N), the reference's per-object
    EllipticalShapeLoss value; all float32.  status (N) uint8: 0 analysed, 1 fewer than min_pixels pixels (skipped, as the reference
    skips them), 2 too large for exact moments (area * (max(w, h) - 1)^4 >= 2^64).  Rows with status != 0 hold the centroid and
    zeros.

    `term` is the reference's formula, and it does NOT vanish for an ellipse: a perfectly filled one scores about 7/3 (2.33 for a
    rasterised ellipse, 2.60 for a square, 2.53 for two touching discs).  To tell a single fruit from a merged cluster or a
    leaf-shaped false positive, read `fill` (1 for a filled ellipse, lower for hollow, merged or ragged shapes) and `axes`."""
    centroid: torch.Tensor
    cov: torch.Tensor
    axes: torch.Tensor
    angle: torch.Tensor
    fill: torch.Tensor
    term: torch.Tensor
    status: torch.Tensor
    offsets: torch.Tensor      # the table's offsets (B + 1) and class_id (N): what loss() needs of it
    class_id: torch.Tensor

    @property
    def valid(self) -> torch.Tensor:
        return self.status == 0

    def loss(self, keep_class=None) -> torch.Tensor:
        """EllipticalShapeLoss over the instances: the mean of `term` over the analysed objects (of class keep_class, when given), 0
        when there are none -- a 0-d float32 device tensor, summed on the device in a fixed order (no host synchronisation)."""
        out = torch.empty((), device=self.term.device, dtype=torch.float32)
        _lib.call("mgu_elliptical_shape_loss_objects", out.device, self.offsets.numel() - 1, self.offsets, self.status.numel(), self.term,
                  self.status, None if keep_class is None else self.class_id, 0 if keep_class is None else int(keep_class), out)
        return out


def _shapes(labels, B, H, W, offsets, capacity, area, bbox, sums, epsilon, min_pixels, out=None, moments=None):
    """Moments and shape of the objects at rows < capacity of the per-object arrays (capacity may be a worst-case bound: rows past
    offsets[B] are left alone).  out: (centroid, cov, axes, angle, fill, term, status) buffers and moments: the int64 (capacity, 12)
    power-sum buffer (uint64 bit patterns), each of capacity rows; allocated when None -- a caller with worst-case buffers keeps
    them across calls, as YieldEvaluator keeps its own."""
    dev = labels.device
    if out is None:
        mk = lambda shape, dt=torch.float32: torch.empty(shape, device=dev, dtype=dt)  # noqa: E731
        out = (mk((capacity, 2)), mk((capacity, 3)), mk((capacity, 2)), mk(capacity), mk(capacity), mk(capacity), mk(capacity, torch.uint8))
    if moments is None:
        moments = torch.empty((capacity, 12), device=dev, dtype=torch.int64)
    _lib.call("mgu_object_moments", dev, labels, B, H, W, offsets, int(capacity), bbox, moments)
    _lib.call("mgu_object_shapes", dev, labels, B, H, W, offsets, int(capacity), area, bbox, sums, moments, float(epsilon), int(min_pixels), *out)
    return out


def object_shapes(table: ObjectTable, epsilon: float = 1e-6, min_pixels: int = 10) -> ObjectShapes:
    """Shape of every object of `table` (mgunet.connected_components) straight from its label map: one pass accumulates exact
    integer moments per object, one thread per object turns them into centroid, covariance, fitted ellipse, fill ratio and the
    reference's per-object EllipticalShapeLoss term (model/unet/shape_loss.py:161-176; epsilon and min_pixels as there); the term of
    a thin object, whose covariance is too ill-conditioned for that closed form, comes from a per-pixel pass.  A fixed number of
    launches whatever the objects, no dense masks, no host synchronisation; results are bitwise repeatable."""
    _lib.require_hip(table.labels, "object_shapes")
    if epsilon < 0 or min_pixels < 0:
        raise ValueError("epsilon and min_pixels must be >= 0")
    B, H, W = table.labels.shape
    N = table.area.numel()
    out = _shapes(table.labels, B, H, W, table.offsets, N, table.area, table.bbox, table.sums, epsilon, min_pixels)
    return ObjectShapes(*out, table.offsets, table.class_id)


def _iou(b1, b2) -> float:
    """IoU of two [xmin, ymin, xmax, ymax] boxes, with the operation order of metrics.py:142-157."""
    iw = max(0, min(b1[2], b2[2]) - max(b1[0], b2[0]))
    ih = max(0, min(b1[3], b2[3]) - max(b1[1], b2[1]))
    inter = iw * ih
    if inter == 0:
        return 0.0
    a1 = (b1[2] - b1[0]) * (b1[3] - b1[1])
    a2 = (b2[2] - b2[0]) * (b2[3] - b2[1])
    return inter / (a1 + a2 - inter)


def _match_host(gt_objects_list, pred_objects_list, thresh):
    """The greedy loop of metrics.py:215-240: (total GT, matched GT, occluded GT, matched occluded GT)."""
    n_gt = n_match = n_occ = n_occ_match = 0
    for gts, preds in zip(gt_objects_list, pred_objects_list):
        used = [False] * len(gts)
        n_gt += len(gts)
        n_occ += sum(1 for o in gts if o.get("occluded", False))
        for p in sorted(preds, key=lambda o: o.get("confidence", 1.0), reverse=True):
            best, best_j = 0, -1
            for j, g in enumerate(gts):
                if not used[j] and g["class_id"] == p["class_id"]:
                    iou = _iou(p["bbox"], g["bbox"])
                    if iou > best:
                        best, best_j = iou, j
            if best >= thresh and best_j != -1:
                used[best_j] = True
                n_match += 1
                if gts[best_j].get("occluded", False):
                    n_occ_match += 1
    return n_gt, n_match, n_occ, n_occ_match


def _yield_dict(gt_counts, pred_counts, match, smooth) -> dict:
    """The arithmetic of metrics.py:178-253 given the matching totals (None: no object lists)."""
    gt_counts = np.array(gt_counts)
    pred_counts = np.array(pred_counts)
    count_accuracy = (1.0 - np.abs(np.sum(pred_counts) - np.sum(gt_counts)) / (np.sum(gt_counts) + smooth)) * 100
    valid = gt_counts > 0
    if np.any(valid):
        yield_error = np.mean(np.abs((gt_counts[valid] - pred_counts[valid]) / gt_counts[valid])) * 100
    else:
        yield_error = 0 if np.sum(np.abs(gt_counts - pred_counts)) == 0 else float("inf")
    matching_rate, occlusion = -1.0, -1.0
    if match is not None:
        n_gt, n_match, n_occ, n_occ_match = match
        matching_rate = (n_match / (n_gt + smooth)) * 100
        occlusion = (n_occ_match / (n_occ + smooth)) * 100 if n_occ > 0 else -1.0
    return {"count_accuracy_perc": count_accuracy, "yield_estimation_error_perc": yield_error,
            "object_matching_rate_perc": matching_rate, "occlusion_robustness_perc": occlusion,
            "total_gt_count_sum": np.sum(gt_counts), "total_pred_count_sum": np.sum(pred_counts)}


def yield_estimation_metrics(gt_counts, pred_counts, gt_objects_list=None, pred_objects_list=None, matching_iou_thresh=0.5,
                             smooth=1e-6) -> dict:
    """experiments/metrics.py:160-253 yield_estimation_metrics: same arguments, same dictionary, same arithmetic (host numpy).
    The reference reads an undefined `smooth` (NameError); here it is a keyword with segmentation_metrics' default 1e-6.  Boxes are
    [xmin, ymin, xmax, ymax]; occlusion_robustness_perc stays -1.0 unless a GT object carries 'occluded': True."""
    match = None
    if gt_objects_list and pred_objects_list:
        match = _match_host(gt_objects_list, pred_objects_list, matching_iou_thresh)
    return _yield_dict(gt_counts, pred_counts, match, smooth)


class _ObjectEvaluator(_Evaluator):
    """What YieldEvaluator and InstanceEvaluator (instances.py) add to the evaluator base: the checks of the object parameters and the
    objects of a batch's two sides."""

    def __init__(self, num_classes, device, connectivity, min_area, split, clean=None):
        _check_args(connectivity, min_area)
        self._clean = None
        if clean is not None:
            extra = set(clean) - {"close_radius", "fill_holes", "max_hole_area", "open_radius"}
            if extra:
                raise ValueError(f"clean takes close_radius, fill_holes, max_hole_area and open_radius, not {sorted(extra)}")
            self._clean = _clean_params(**clean)
            if not 2 <= int(num_classes) <= 32:
                raise ValueError("clean needs 2 <= num_classes <= 32")
        self._split = None
        if split is not None:
            extra = set(split) - {"min_distance", "min_radius", "min_area"}
            if extra:
                raise ValueError(f"split takes min_distance, min_radius and min_area, not {sorted(extra)}")
            self._split = _split_params(split.get("min_distance", 5), split.get("min_radius", 3), split.get("min_area", 0))
        super().__init__(num_classes, device)
        self.connectivity, self.min_area = connectivity, int(min_area)
        self._bufs, self._cap = None, -1

    def _label_sides(self, src, masks, B, H, W, C, bufs):
        """Label, split (when asked) and take the statistics of the GT objects (mask values in [1, num_classes)) and of the predicted
        objects (argmax fused, min_area) into bufs[side] = (labels, class, bbox[, area]), worst-case buffers of self._cap rows: no
        host synchronisation.  With `clean`, the predicted side is the cleaned class map (bufs["clean"], mgunet.clean_masks) in the
        place of the logits; the GT stays as annotated.  Returns the two sides' counts and offsets."""
        counts, offsets = {}, {}
        pred = (src, 1, C, 0)
        if self._clean is not None:
            cm = bufs["clean"][:B * H * W].view(B, H, W)
            _clean(src, 1, B, H, W, C, C, self._clean, cm)
            pred = (cm, 0, 0, self.num_classes)
        for side, s, k, cc, ncls, amin in (("gt", masks, 0, 0, self.num_classes, 0), ("pred", *pred, self.min_area)):
            lab, cls, bbox, *area = bufs[side]
            lab = lab[:B * H * W].view(B, H, W)
            counts[side] = torch.empty(B, device=self.device, dtype=torch.int64)
            offsets[side] = torch.empty(B + 1, device=self.device, dtype=torch.int64)
            _label(s, k, B, H, W, cc, self.connectivity, 0, ncls, amin, lab, counts[side], offsets[side])
            if self._split is not None:   # in place: the split has read the components before it writes the objects
                _split(lab, B, H, W, self._split, lab, counts[side], offsets[side])
            _stats(lab, s, k, B, H, W, cc, offsets[side], self._cap, cls, bbox, *area)
        return counts, offsets


class YieldEvaluator(_ObjectEvaluator):
    """Device-side yield estimation over a test set.  update(logits, masks) labels the predicted objects (argmax fused into the
    labelling) and the GT objects (mask values in [1, num_classes); 0, -100 and anything out of range are background), appends the
    per-image counts to device buffers and accumulates the matching totals; it never blocks the host.  min_area applies to the
    predicted objects.  compute() synchronises once and returns yield_estimation_metrics' dictionary -- equal to calling it on the
    per-image counts and to_dicts() of the same batches.  split: a dict of split_objects' min_distance / min_radius / min_area; the
    predicted and the GT objects alike are then cut apart (mgunet.split_objects) before they are counted and matched, still without
    a host synchronisation.  None: objects are the connected components.  clean: a dict of clean_masks' close_radius / fill_holes /
    max_hole_area / open_radius; the predicted class map is then cleaned (mgunet.clean_masks) before it is labelled (min_area) and
    split -- the GT stays as annotated -- still without a host synchronisation.  None: the argmax map is labelled as it is."""

    def __init__(self, num_classes: int, device, connectivity: int = 2, min_area: int = 0, iou_thresh: float = 0.5, smooth: float = 1e-6,
                 split: dict = None, clean: dict = None):
        super().__init__(num_classes, device, connectivity, min_area, split, clean)
        self.iou_thresh, self.smooth = float(iou_thresh), smooth
        self.reset()

    def reset(self) -> None:
        self.totals = torch.zeros(3, device=self.device, dtype=torch.int64)   # GT objects, predicted objects, matched GT objects
        self.gt_counts, self.pred_counts = [], []

    def _buffers(self, B, H, W):
        n = B * H * W
        if n > self._cap:   # per-object arrays sized for the worst case (every pixel its own object): no host synchronisation
            mk = lambda shape, dt: torch.empty(shape, device=self.device, dtype=dt)  # noqa: E731
            self._bufs = {s: (mk(n, torch.int32), mk(n, torch.int64), mk((n, 4), torch.int32)) for s in ("gt", "pred")}
            if self._clean is not None:
                self._bufs["clean"] = mk(n, torch.int64)
            self._cap = n
        return self._bufs

    def update(self, logits_nchw: torch.Tensor, masks: torch.Tensor) -> None:
        """Add one batch: logits (B, C, H, W) float32 -- the view UNet.forward returns -- and integer masks (B, H, W)."""
        src, masks, B, H, W, C = self._batch(logits_nchw, masks)
        bufs = self._buffers(B, H, W)
        counts, offsets = self._label_sides(src, masks, B, H, W, C, bufs)
        (gl, gc, gb), (pl, pc, pb) = bufs["gt"], bufs["pred"]
        _lib.call("mgu_match_objects", self.device, B, offsets["gt"], gc, gb, self._cap, offsets["pred"], pc, pb, self._cap, self.iou_thresh,
                  self.totals)
        self.gt_counts.append(counts["gt"])
        self.pred_counts.append(counts["pred"])

    def compute(self) -> dict:
        """Synchronise once and return yield_estimation_metrics' dictionary over every batch since the last reset()."""
        if not self.gt_counts:
            return yield_estimation_metrics([], [], smooth=self.smooth)
        gt = torch.cat(self.gt_counts).cpu().tolist()
        pred = torch.cat(self.pred_counts).cpu().tolist()
        n_gt, _, n_match = self.totals.cpu().tolist()
        return _yield_dict(gt, pred, (n_gt, n_match, 0, 0), self.smooth)


def evaluate_yield(model, loader, num_classes=None, connectivity=2, min_area=0, iou_thresh=0.5, smooth=1e-6, split=None, clean=None) -> dict:
    """Yield estimation over `loader`'s (images, masks) batches: logits = model(images) under torch.no_grad() in eval mode, the
    predicted class map cleaned (with `clean`), objects labelled (and, with `split`, cut apart: see YieldEvaluator) and matched on the
    device.  Returns yield_estimation_metrics' dictionary; the model's training flag is restored."""
    return _evaluate(model, loader, num_classes, lambda C, dev: YieldEvaluator(
        C, dev, connectivity=connectivity, min_area=min_area, iou_thresh=iou_thresh, smooth=smooth, split=split, clean=clean))
