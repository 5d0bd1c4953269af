"""Segmentation evaluation: replaces experiments/metrics.py:6-69 (segmentation_metrics) and the scoring loop of
experiments/segmentation_performance.py:125-151.

The reference copies every prediction and mask of the test set to the host and builds an sklearn confusion matrix.  Here the
argmax, the confusion counts and (optionally) the validation loss come out of ONE pass over the logits and masks on the device
(mgu_segmentation_eval), accumulated across batches in an int64 (C, C) buffer without a host synchronisation; the host only
turns the C x C counts into the reference's dictionary, with the reference's own operation order (bitwise equal results).
There is no sklearn dependency."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._args import logits_and_masks, resolve_device

_LOSS_KINDS = {None: 0, "ce": 1, "ce+dice": 2}


def metrics_from_confusion(cm, smooth=1e-6) -> dict:
    """The arithmetic of segmentation_metrics (metrics.py:27-68) on a (C, C) int64 confusion matrix (rows: truth, columns:
    prediction), in the reference's operation order: per-class values are np.float64, means np.nanmean (NaN per-class values,
    possible with smooth = 0, are skipped as there)."""
    cm = np.asarray(cm)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1]:
        raise ValueError(f"expected a square confusion matrix, got shape {cm.shape}")
    cm = cm.astype(np.int64, copy=False)
    iou_per_class, precision_per_class, recall_per_class, f1_per_class = [], [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for cls_idx in range(cm.shape[0]):
            tp = cm[cls_idx, cls_idx]
            fp = np.sum(cm[:, cls_idx]) - tp
            fn = np.sum(cm[cls_idx, :]) - tp
            iou = (tp + smooth) / (tp + fp + fn + smooth)
            precision = (tp + smooth) / (tp + fp + smooth)
            recall = (tp + smooth) / (tp + fn + smooth)
            f1 = (2 * precision * recall + smooth) / (precision + recall + smooth)
            iou_per_class.append(iou)
            precision_per_class.append(precision)
            recall_per_class.append(recall)
            f1_per_class.append(f1)
    import warnings
    with warnings.catch_warnings():   # an all-NaN list: np.nanmean returns NaN (and warns) exactly as in the reference
        warnings.simplefilter("ignore", RuntimeWarning)
        means = [np.nanmean(v) for v in (iou_per_class, precision_per_class, recall_per_class, f1_per_class)]
    return {"iou_per_class": iou_per_class, "precision_per_class": precision_per_class, "recall_per_class": recall_per_class,
            "f1_per_class": f1_per_class, "mean_iou": means[0], "mean_precision": means[1], "mean_recall": means[2],
            "mean_f1": means[3], "confusion_matrix": cm}


def confusion_matrix_host(true_flat, pred_flat, num_classes: int) -> np.ndarray:
    """sklearn.metrics.confusion_matrix(true, pred, labels=range(num_classes)) with numpy: pairs with a label outside
    [0, num_classes) on either side are dropped, as sklearn drops them."""
    t = np.asarray(true_flat).reshape(-1).astype(np.int64)
    p = np.asarray(pred_flat).reshape(-1).astype(np.int64)
    C = int(num_classes)
    keep = (t >= 0) & (t < C) & (p >= 0) & (p < C)
    return np.bincount(t[keep] * C + p[keep], minlength=C * C).astype(np.int64).reshape(C, C)


def confusion_matrix_device(true_flat: torch.Tensor, pred_flat: torch.Tensor, num_classes: int, out: torch.Tensor = None) -> torch.Tensor:
    """The same counts on the device (mgu_confusion_matrix), accumulated into `out` (int64 (C, C), zeros if not given)."""
    dev = true_flat.device
    t = true_flat.reshape(-1).to(torch.int64).contiguous()
    p = pred_flat.to(dev).reshape(-1).to(torch.int64).contiguous()
    C = int(num_classes)
    if out is None:
        out = torch.zeros((C, C), device=dev, dtype=torch.int64)
    _lib.call("mgu_confusion_matrix", dev, t, p, t.numel(), C, out)
    return out


def segmentation_metrics(true_masks_flat, pred_masks_flat, num_classes, smooth=1e-6) -> dict:
    """experiments/metrics.py:6-69 segmentation_metrics: same arguments, same dictionary.  Device tensors are counted on the
    device (mgu_confusion_matrix); host arrays / tensors with numpy."""
    C = int(num_classes)
    if C < 1:
        raise ValueError("'labels' should contains at least one label.")
    on_dev = any(isinstance(v, torch.Tensor) and v.is_cuda for v in (true_masks_flat, pred_masks_flat))
    if on_dev:
        dev = true_masks_flat.device if isinstance(true_masks_flat, torch.Tensor) and true_masks_flat.is_cuda else pred_masks_flat.device
        t = torch.as_tensor(true_masks_flat).to(dev).reshape(-1)
        p = torch.as_tensor(pred_masks_flat).to(dev).reshape(-1)
        if t.numel() != p.numel():
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{t.numel()}, {p.numel()}]")
        any_label = t.numel() == 0 or bool(((t >= 0) & (t < C)).any())
        cm = confusion_matrix_device(t, p, C).cpu().numpy()
    else:
        t = true_masks_flat.cpu().numpy() if isinstance(true_masks_flat, torch.Tensor) else np.asarray(true_masks_flat)
        p = pred_masks_flat.cpu().numpy() if isinstance(pred_masks_flat, torch.Tensor) else np.asarray(pred_masks_flat)
        t, p = t.reshape(-1), p.reshape(-1)
        if t.size != p.size:
            raise ValueError(f"Found input variables with inconsistent numbers of samples: [{t.size}, {p.size}]")
        any_label = t.size == 0 or bool(((t >= 0) & (t < C)).any())
        cm = confusion_matrix_host(t, p, C)
    if not any_label:   # sklearn's confusion_matrix raises here
        raise ValueError("At least one label specified must be in y_true")
    return metrics_from_confusion(cm, smooth)


def allreduce_eval_state(confusion: torch.Tensor, loss_acc: torch.Tensor = None, group=None):
    """SUM of the int64 confusion counts (and of the double[2] loss accumulator) over the ranks of `group`; returns new tensors
    (the inputs are left as they are).  Integer counts: data-parallel evaluation equals single-process evaluation exactly.
    One process, or torch.distributed not initialised: copies of the inputs.  Works on CPU tensors (gloo) and on device
    tensors (any backend; with gloo the device tensors travel through the host)."""
    import torch.distributed as dist
    cm = confusion.clone()
    acc = loss_acc.clone() if loss_acc is not None else None
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return cm, acc
    for t in (cm, acc):
        if t is None:
            continue
        if t.is_cuda and dist.get_backend(group) == "gloo":
            host = t.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            t.copy_(host)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return cm, acc


class _Evaluator:
    """What the evaluators share -- SegmentationEvaluator, BoundaryEvaluator and, through objects._ObjectEvaluator, YieldEvaluator
    and InstanceEvaluator: the class count and device of the constructor, the checks of update()'s batch, and the contract _evaluate
    relies on: reset() forgets every batch, update(logits, masks) adds one without blocking the host, compute() synchronises and
    returns the dictionary."""

    CLASS_RANGE = (1, None)   # num_classes a subclass takes: (least, most or None)

    def __init__(self, num_classes, device):
        self.num_classes = int(num_classes)
        lo, hi = self.CLASS_RANGE
        if self.num_classes < lo or (hi is not None and self.num_classes > hi):
            raise ValueError(f"num_classes must be >= {lo}" if hi is None else f"num_classes must be in {lo}..{hi}, got {num_classes}")
        self.device = resolve_device(device, type(self).__name__)

    def _batch(self, logits_nchw, masks):
        """(NHWC logits, int64 masks on the device, B, H, W, C) of update()'s arguments, checked."""
        return logits_and_masks(logits_nchw, masks, self.device, self.num_classes)

    def reset(self) -> None:
        raise NotImplementedError

    def update(self, logits_nchw: torch.Tensor, masks: torch.Tensor):
        raise NotImplementedError

    def compute(self) -> dict:
        raise NotImplementedError


class SegmentationEvaluator(_Evaluator):
    """Device-side accumulation of the reference's evaluation (segmentation_performance.py:125-151) and of a validation loss
    (the block train_segmentation.py:145-151 leaves commented out).  update() never blocks the host; compute() synchronises
    once and returns segmentation_metrics' dictionary (+ 'loss': the mean per-batch loss when a loss was requested)."""

    def __init__(self, num_classes: int, device, loss=None, dice_smooth: float = 1.0, smooth: float = 1e-6):
        if loss not in _LOSS_KINDS:
            raise ValueError(f"unknown loss {loss!r}: None, 'ce' or 'ce+dice'")
        super().__init__(num_classes, device)
        self.loss, self.loss_kind = loss, _LOSS_KINDS[loss]
        self.dice_smooth, self.smooth = float(dice_smooth), smooth
        self.confusion = torch.zeros((self.num_classes, self.num_classes), device=self.device, dtype=torch.int64)
        self.loss_acc = torch.zeros(2, device=self.device, dtype=torch.float64) if self.loss_kind else None

    def reset(self) -> None:
        self.confusion.zero_()
        if self.loss_acc is not None:
            self.loss_acc.zero_()

    def update(self, logits_nchw: torch.Tensor, masks: torch.Tensor, return_pred: bool = False):
        """Add one batch: logits (B, C, H, W) -- the view UNet.forward returns, its NHWC storage read in place -- and int64 masks
        (B, H, W).  Returns the (B, H, W) int64 predictions if return_pred (= torch.argmax(logits, 1)), else None."""
        nhwc, masks, B, H, W, Cc = self._batch(logits_nchw, masks)
        pred = torch.empty((B, H, W), device=self.device, dtype=torch.int64) if return_pred else None
        _lib.call("mgu_segmentation_eval", self.device, nhwc, masks, B, H * W, Cc, self.confusion, pred, self.loss_kind, self.dice_smooth,
                  self.loss_acc)
        return pred

    def compute(self, group=None) -> dict:
        """Synchronise, raise ValueError if a loss kernel met an invalid label (as losses.check_labels), SUM the counts and loss
        accumulators over the ranks of `group` when torch.distributed runs more than one, and return the reference's dictionary."""
        _lib.call("mgu_loss_sync_check", self.device)
        cm, acc = allreduce_eval_state(self.confusion, self.loss_acc, group)
        res = metrics_from_confusion(cm.cpu().numpy(), self.smooth)
        if acc is not None:
            a = acc.cpu().numpy()
            res["loss"] = float(a[0] / a[1]) if a[1] > 0 else float("nan")
        return res


def _evaluate(model, loader, num_classes, make_evaluator) -> dict:
    """The loop the evaluate_* functions share: ev = make_evaluator(classes, device), then for each (images, masks) batch of `loader`
    logits = model(images) under torch.no_grad() in eval mode and ev.update(logits, masks); returns ev.compute().  The classes default
    to model.num_classes; the model's training flag is restored."""
    dev = next(model.parameters()).device
    ev = make_evaluator(int(num_classes if num_classes is not None else model.num_classes), dev)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for images, masks in loader:
                out = model(images.to(dev))
                logits = out[0] if isinstance(out, (tuple, list)) else out
                ev.update(logits, masks.to(dev))
        return ev.compute()
    finally:
        model.train(was_training)


def evaluate_segmentation(model, loader, num_classes=None, loss=None, smooth=1e-6) -> dict:
    """The evaluation loop of segmentation_performance.py:125-151 (no file I/O): for each (images, masks) batch of `loader`,
    logits = model(images) under torch.no_grad() in eval mode, then argmax + confusion counts (+ loss) on the device.  Returns
    segmentation_metrics' dictionary over the whole loader (+ 'loss').  The model's training flag is restored afterwards, so a
    training script can validate between epochs (also on a model whose parameters a Trainer has re-homed)."""
    return _evaluate(model, loader, num_classes, lambda C, dev: SegmentationEvaluator(C, dev, loss=loss, smooth=smooth))
