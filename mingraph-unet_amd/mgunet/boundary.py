"""Boundary evaluation: how well the predicted outline of every class follows the true one -- the BF score (Csurka et al. 2013),
Boundary IoU (Cheng et al. 2021), Hausdorff distance, its 95th percentile and the average symmetric surface distance.  The reference
has no boundary metric (experiments/metrics.py stops at region metrics and box matching); the definitions are this build's own.

Everything per pixel runs on the device in integers (csrc/boundary.hip, mgu_boundary_tables): boundary_tables gives, per image and
foreground class, the histogram of the squared surface distances in both directions, their count / unmatched / maximum / fixed-point
sum of roots, and the band counts.  boundary_metrics turns such tables into the dictionary on the host, in float64: the only place
where floats appear, so tables from the device and from an oracle give == dictionaries.  BoundaryEvaluator accumulates over batches
without a host synchronisation.

With X one of the two class maps of an image (P the prediction, G the target) and c a foreground class 1 .. num_classes - 1 (every
other value, 0, -100 or out of range, reads as background on both sides):
  boundary   dX_c = the pixels of class c in X with a 4-neighbour inside the image holding another value.  Pixels outside the image do
             not count, as in distance_transform and the opening of clean_masks: a fruit cut by the frame has no contour along the
             frame, a map that is entirely class c has an empty boundary.  (The published Boundary IoU code pads with background and
             so differs here.)
  distance   direction 0: for p in dP_c, d2(p) = min |p - q|^2 over q in dG_c, exact; p is unmatched when dG_c is empty in its image.
             Direction 1 is the converse.
  band       X_c^r = {p of class c in X : D2_X(p) <= band_r2}, D2_X = distance_transform of X: a Euclidean disc, not the paper's
             iterated 3 x 3 erosion."""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from ._args import batched_map
from .metrics import _Evaluator, _evaluate
from .objects import _source

_NAN = float("nan")   # the one nan object of every dictionary: lists and dictionaries compare by identity first, so equal tables give == results
MAX_D2 = 4096   # the largest histogram mgu_boundary_tables takes: max_distance <= 64


@dataclass
class BoundaryTables:
    """mgu_boundary_tables' three int64 tables of B images and K = num_classes - 1 foreground classes (class c at index c - 1), device
    tensors from boundary_tables (numpy arrays from an oracle do as well for boundary_metrics).  hist (B, K, 2, max_d2 + 2): per
    direction (0 prediction -> target, 1 target -> prediction), bin k <= max_d2 counts the source boundary pixels with d2 == k, the last
    bin those with d2 > max_d2 plus the unmatched ones.  stats (B, K, 2, 4): [n source boundary pixels, n unmatched, max d2 over the
    matched pixels (0 if none), sum over the matched pixels of floor(2^16 sqrt(d2)) = math.isqrt(d2 << 32)].  band (B, K, 3):
    [|P^r & G^r|, |P^r|, |G^r|].  band_r2 is None for tables concatenated from images of different sizes."""
    hist: torch.Tensor
    stats: torch.Tensor
    band: torch.Tensor
    max_d2: int
    band_r2: int


def _max_d2(max_distance) -> int:
    """floor(max_distance^2), 1..4096 (a hair is added before the floor, as clean_masks squares its radii)"""
    if not max_distance >= 1:
        raise ValueError("max_distance must be >= 1")
    d2 = math.floor(max_distance * max_distance + 1e-9)
    if d2 > MAX_D2:
        raise ValueError(f"max_distance {max_distance}: the squared distance must stay within {MAX_D2}")
    return d2


def _band_r2(band_radius, H, W) -> int:
    """floor(band_radius^2), at least 1; None: 2 % of the image diagonal, as in Cheng et al."""
    if band_radius is None:
        band_radius = 0.02 * math.hypot(H, W)
    elif not band_radius > 0:
        raise ValueError("band_radius must be > 0")
    return min(max(1, math.floor(band_radius * band_radius + 1e-9)), 2 ** 31 - 1)


def _tol2(tolerance, max_d2) -> int:
    if not tolerance >= 0:
        raise ValueError("tolerance must be >= 0")
    t2 = math.floor(tolerance * tolerance + 1e-9)
    if t2 > max_d2:
        raise ValueError(f"tolerance {tolerance}: its square must stay within max_d2 = {max_d2} (raise max_distance)")
    return t2


def _rank_fraction(quantile) -> Fraction:
    if not 0 < quantile <= 1:
        raise ValueError("quantile must be in (0, 1]")
    return Fraction(quantile).limit_denominator(10 ** 6)


def _tables(src, kind, target, B, H, W, C, ncls, max_d2, band_r2):
    """mgu_boundary_tables on checked arguments: the three tables (zero for a batch without pixels, which the call does not touch)"""
    dev, K = src.device, ncls - 1
    hist = torch.zeros((B, K, 2, max_d2 + 2), device=dev, dtype=torch.int64)
    stats = torch.zeros((B, K, 2, 4), device=dev, dtype=torch.int64)
    band = torch.zeros((B, K, 3), device=dev, dtype=torch.int64)
    if B * H * W:   # a batch without pixels has no storage to point at
        _lib.call("mgu_boundary_tables", dev, src, kind, target, B, H, W, C, ncls, max_d2, band_r2, hist, stats, band)
    return hist, stats, band


def boundary_tables(pred: torch.Tensor, target: torch.Tensor, num_classes: int = None, max_distance: float = 64,
                    band_radius: float = None) -> BoundaryTables:
    """The integer tables behind the boundary metrics of a batch, on the device (the module docstring states the definitions).

    pred: whatever clean_masks takes -- an integer class map (H, W) or (B, H, W), for which num_classes is required, or (B, C, H, W)
    float32 logits (argmax fused, first maximal class; num_classes is C).  target: an integer (H, W) or (B, H, W) map of the same
    size.  An (H, W) input is a batch of one.  max_d2 = floor(max_distance^2) <= 4096 is the last exact histogram bin;
    band_r2 = floor(band_radius^2), at least 1, band_radius None meaning 2 % of the image diagonal.  Six launches and three fills, no
    host synchronisation; bitwise repeatable.  H, W <= 16384, B <= 32767, 2B (HW + 1) < 2^31."""
    max_d2 = _max_d2(max_distance)
    if band_radius is not None:
        _band_r2(band_radius, 1, 1)
    src, kind, B, H, W, C = _source(pred)
    if kind == 0 and num_classes is None:
        raise ValueError("boundary_tables: num_classes is required for a class map")
    ncls = C if kind == 1 else int(num_classes)
    if num_classes is not None and int(num_classes) != ncls:
        raise ValueError(f"boundary_tables: logits have {C} classes, num_classes is {num_classes}")
    if not 2 <= ncls <= 32:
        raise ValueError(f"boundary_tables: num_classes must be in 2..32, got {ncls}")
    _lib.require_hip(target, "boundary_tables")
    tgt = batched_map(target, "the target")
    if tuple(tgt.shape) != (B, H, W):
        raise ValueError(f"target shape {tuple(target.shape)} does not match the prediction's {(B, H, W)}")
    if tgt.device != src.device:
        raise RuntimeError(f"the target must live on {src.device}")
    band_r2 = _band_r2(band_radius, H, W)
    return BoundaryTables(*_tables(src, kind, tgt.to(torch.int64).contiguous(), B, H, W, C, ncls, max_d2, band_r2), max_d2, band_r2)


def _ratio(num, den) -> float:
    return float(num) / float(den) if den else _NAN


def _mean(values) -> float:
    values = [v for v in values if not math.isnan(v)]
    return float(np.mean(np.array(values, np.float64))) if values else _NAN


def boundary_metrics(tables: BoundaryTables, tolerance: float = 2.0, quantile: float = 0.95) -> dict:
    """The boundary metrics of BoundaryTables (device tensors or numpy arrays), on the host in float64.  Every per-class entry is a
    list over the foreground classes 1 .. K; an undefined ratio is nan.
      bf_precision, bf_recall, bf_score   pooled over all images: the direction-0 (direction-1) boundary pixels with
                     d2 <= floor(tolerance^2) over all of them, and their harmonic mean (0 when both are 0).  tolerance^2 must stay
                     within the tables' max_d2 (ValueError).
      boundary_iou   pooled: inter / (|P^r| + |G^r| - inter) of the band counts.
      hausdorff, hd95, assd   per image, then averaged over the images where the class has a boundary on both sides (`images` of
                     them): sqrt of the larger directed maximum; sqrt of the larger directed quantile, the smallest k whose cumulative
                     count reaches ceil(quantile n) (the rank in integers) -- when that rank falls into the overflow bin the
                     direction's exact maximum stands in, an upper bound, and the image is counted in hd95_saturated;
                     (S0 + S1) / 2^16 / (n0 + n1) of the fixed-point sums.
      missing        images where exactly one side has a boundary of the class: left out of the three distance means, but part of the
                     pooled counts (their pixels are unmatched).  An image where neither side has one is skipped.
      mean_<name>    the mean over the classes where <name> is defined."""
    to_np = lambda t: np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t).astype(np.int64)  # noqa: E731
    hist, stats, band = to_np(tables.hist), to_np(tables.stats), to_np(tables.band)
    max_d2 = int(tables.max_d2)
    B, K = stats.shape[:2]
    if hist.shape != (B, K, 2, max_d2 + 2) or stats.shape != (B, K, 2, 4) or band.shape != (B, K, 3):
        raise ValueError(f"tables of shapes {hist.shape}, {stats.shape}, {band.shape} for max_d2 = {max_d2}")
    t2 = _tol2(tolerance, max_d2)
    q = _rank_fraction(quantile)
    names = ("bf_precision", "bf_recall", "bf_score", "boundary_iou", "hausdorff", "hd95", "assd")
    out = {k: [] for k in names + ("images", "missing", "hd95_saturated")}
    for k in range(K):
        within = hist[:, k, :, :t2 + 1].sum(axis=(0, 2))
        total = stats[:, k, :, 0].sum(axis=0)
        p, r = _ratio(within[0], total[0]), _ratio(within[1], total[1])
        out["bf_precision"].append(p)
        out["bf_recall"].append(r)
        out["bf_score"].append(_NAN if math.isnan(p) or math.isnan(r) else (2 * p * r / (p + r) if p + r else 0.0))
        inter, ap, ag = (int(v) for v in band[:, k].sum(axis=0))
        out["boundary_iou"].append(_ratio(inter, ap + ag - inter))
        hd, hq, asd, missing, saturated = [], [], [], 0, 0
        for b in range(B):
            n = [int(stats[b, k, d, 0]) for d in (0, 1)]
            if not n[0] or not n[1]:
                missing += bool(n[0] or n[1])
                continue
            hd.append(math.sqrt(max(int(stats[b, k, 0, 2]), int(stats[b, k, 1, 2]))))
            worst, sat = 0, False
            for d in (0, 1):
                rank = max(1, (q.numerator * n[d] + q.denominator - 1) // q.denominator)
                at = int(np.searchsorted(np.cumsum(hist[b, k, d, :max_d2 + 1]), rank))   # the first bin whose cumulative count reaches it
                if at > max_d2:
                    at, sat = int(stats[b, k, d, 2]), True
                worst = max(worst, at)
            hq.append(math.sqrt(worst))
            saturated += sat
            asd.append((int(stats[b, k, 0, 3]) + int(stats[b, k, 1, 3])) / 65536 / (n[0] + n[1]))
        for name, vals in (("hausdorff", hd), ("hd95", hq), ("assd", asd)):
            out[name].append(_mean(vals))
        out["images"].append(len(hd))
        out["missing"].append(missing)
        out["hd95_saturated"].append(saturated)
    for name in names:
        out["mean_" + name] = _mean(out[name])
    return out


class BoundaryEvaluator(_Evaluator):
    """Device-side boundary evaluation over a test set.  update(logits, masks) runs boundary_tables on the batch (argmax fused; mask
    values in [1, num_classes) are foreground, 0, -100 and anything out of range background) and keeps its tables on the device; it
    never blocks the host.  compute() concatenates them, synchronises once and returns boundary_metrics' dictionary -- equal to
    boundary_metrics of the tables of the concatenated batches.  With band_radius None every batch takes 2 % of its own diagonal.
    One process: reducing the tables across ranks is out of scope (they are per image; gather them, do not add them)."""

    CLASS_RANGE = (2, 32)

    def __init__(self, num_classes: int, device, tolerance: float = 2.0, max_distance: float = 64, band_radius: float = None,
                 quantile: float = 0.95):
        super().__init__(num_classes, device)
        self.max_d2 = _max_d2(max_distance)
        _tol2(tolerance, self.max_d2)
        _rank_fraction(quantile)
        if band_radius is not None:
            _band_r2(band_radius, 1, 1)
        self.tolerance, self.band_radius, self.quantile = tolerance, band_radius, quantile
        self.reset()

    def reset(self) -> None:
        self._tables, self._band_r2 = [], set()

    def update(self, logits_nchw: torch.Tensor, masks: torch.Tensor) -> None:
        """Add one batch: logits (B, C, H, W) float32 -- the view UNet.forward returns -- and integer masks (B, H, W)."""
        src, masks, B, H, W, C = self._batch(logits_nchw, masks)
        band_r2 = _band_r2(self.band_radius, H, W)
        self._tables.append(_tables(src, 1, masks, B, H, W, C, C, self.max_d2, band_r2))
        self._band_r2.add(band_r2)

    def tables(self) -> BoundaryTables:
        """The tables of every batch since the last reset(), concatenated along the images (device tensors; no synchronisation)."""
        K = self.num_classes - 1
        if not self._tables:
            mk = lambda *shape: torch.zeros(shape, device=self.device, dtype=torch.int64)  # noqa: E731
            return BoundaryTables(mk(0, K, 2, self.max_d2 + 2), mk(0, K, 2, 4), mk(0, K, 3), self.max_d2, None)
        hist, stats, band = (torch.cat(t) for t in zip(*self._tables))
        return BoundaryTables(hist, stats, band, self.max_d2, next(iter(self._band_r2)) if len(self._band_r2) == 1 else None)

    def compute(self) -> dict:
        """Synchronise once and return boundary_metrics' dictionary over every batch since the last reset()."""
        return boundary_metrics(self.tables(), self.tolerance, self.quantile)


def evaluate_boundaries(model, loader, num_classes=None, tolerance=2.0, max_distance=64, band_radius=None, quantile=0.95) -> dict:
    """Boundary evaluation over `loader`'s (images, masks) batches: logits = model(images) under torch.no_grad() in eval mode, the
    tables of every batch on the device (see BoundaryEvaluator).  Returns boundary_metrics' dictionary; the model's training flag is
    restored.  One process: no multi-rank reduction."""
    return _evaluate(model, loader, num_classes, lambda C, dev: BoundaryEvaluator(
        C, dev, tolerance=tolerance, max_distance=max_distance, band_radius=band_radius, quantile=quantile))
