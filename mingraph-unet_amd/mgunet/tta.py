"""Test-time augmentation and confidence on the device: predict_tta runs a UNet on flipped / rotated views of a batch and averages the
views' softmax probabilities after undoing each transform; object_scores turns those probabilities into one confidence per object of
a connected_components table (ObjectTable.to_dicts(scores=...) carries it into yield_estimation_metrics, which matches predictions in
the reference's confidence order, experiments/metrics.py:218).

Per shape group, csrc/tta.hip writes the views as one contiguous batch (one launch), the model runs one forward on it, and one merge
launch maps every output pixel into each view, takes the softmax and sums.  The view table below is the single host description of
the transforms: both kernels use its index arithmetic, and tests/test_tta_host.py checks it against torch.flip / torch.rot90."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._args import nhwc_storage
from .objects import ObjectTable
from .unet import UNet

# flip bits: 1 = torch.flip(x, (3,)) (fW), 2 = torch.flip(x, (2,)) (fH), applied before r quarter turns torch.rot90(x, r, (2, 3))
TRANSFORMS = {
    "none": ((0, 0),),
    "hflip": ((0, 0), (1, 0)),
    "flips": ((0, 0), (1, 0), (2, 0), (3, 0)),
    "d4": tuple((0, r) for r in range(4)) + tuple((1, r) for r in range(4)),
}
MAX_CLASSES = 16   # csrc/tta.hip TTA_MAX_C


def view_table(transforms: str, H: int, W: int):
    """(views, groups) of a transform set on H x W images.  views: one (group, slot, flip, turns) per view, in averaging order.
    groups: one (Hv, Wv, [(flip, turns), ...]) per shape group, its views in slot order; group 0 holds the views of shape (H, W) (every
    view when H == W), group 1 those of shape (W, H).  Each group is one forward of slots * B images, view-major."""
    if transforms not in TRANSFORMS:
        raise ValueError(f"unknown transforms {transforms!r}; expected one of {sorted(TRANSFORMS)}")
    groups = [(H, W, []), (W, H, [])]
    views = []
    for flip, r in TRANSFORMS[transforms]:
        g = (r & 1) if H != W else 0
        views.append((g, len(groups[g][2]), flip, r))
        groups[g][2].append((flip, r))
    return views, [grp for grp in groups if grp[2]]


def view_source_index(flip: int, turns: int, H: int, W: int) -> torch.Tensor:
    """int64 (Hv, Wv): for each pixel (i, j) of the view, the linear index y * W + x of the source pixel it shows (csrc/tta.hip
    tta_to_source).  view = x.flatten(-2)[..., idx]."""
    Hv, Wv = (W, H) if turns & 1 else (H, W)
    i = torch.arange(Hv).view(-1, 1).expand(Hv, Wv)
    j = torch.arange(Wv).view(1, -1).expand(Hv, Wv)
    a, b = [(i, j), (j, W - 1 - i), (H - 1 - i, W - 1 - j), (H - 1 - j, i)][turns]
    y = H - 1 - a if flip & 2 else a
    x = W - 1 - b if flip & 1 else b
    return y * W + x


def view_inverse_index(flip: int, turns: int, H: int, W: int) -> torch.Tensor:
    """int64 (H, W): for each source pixel (y, x), the linear index i * Wv + j of the view pixel that shows it (csrc/tta.hip
    tta_to_view, the merge's gather).  x = view.flatten(-2)[..., idx]."""
    Wv = H if turns & 1 else W
    y = torch.arange(H).view(-1, 1).expand(H, W)
    x = torch.arange(W).view(1, -1).expand(H, W)
    a = H - 1 - y if flip & 2 else y
    b = W - 1 - x if flip & 1 else x
    i, j = [(a, b), (W - 1 - b, a), (H - 1 - a, W - 1 - b), (b, H - 1 - a)][turns]
    return i * Wv + j


def _check_model(model):
    if not isinstance(model, UNet):
        raise TypeError(f"predict_tta needs an mgunet.UNet, got {type(model).__name__}")
    if model.training:
        raise RuntimeError("test-time augmentation is an inference mode: call .eval() first")


def predict_tta(model: UNet, images: torch.Tensor, transforms: str = "d4"):
    """Softmax probabilities of `model` averaged over the views of `images` listed in TRANSFORMS[transforms], each mapped back to the
    input's pixels.  images: float32 (B, Cin, H, W) on the HIP device, any strides.  Returns (probs, labels, confidence): probs float32
    (B, C, H, W), an NCHW view of NHWC storage like UNet.forward's logits; labels int64 (B, H, W) = probs.argmax(1); confidence float32
    (B, H, W) = probs.amax(1).  "none" gives the plain forward's softmax."""
    _check_model(model)
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError("expected a (B,C,H,W) tensor")
    _lib.require_hip(images, "predict_tta")
    if images.dtype != torch.float32:
        raise TypeError(f"expected float32 input, got {images.dtype}")
    B, Cin, H, W = images.shape
    if Cin != model.in_channels:
        raise RuntimeError(f"expected {model.in_channels} input channels, got {Cin}")
    Cls = model.num_classes
    if Cls > MAX_CLASSES:
        raise ValueError(f"predict_tta supports at most {MAX_CLASSES} classes, the model has {Cls}")
    views, groups = view_table(transforms, H, W)
    if B == 0 or H == 0 or W == 0:
        raise ValueError("predict_tta needs a non-empty batch")
    dev = images.device
    strides = (C.c_int64 * 4)(*images.stride())
    logits = []
    with torch.no_grad():
        for Hv, Wv, gv in groups:
            if gv == [(0, 0)]:   # the identity alone: the forward reads the caller's image through its strides
                lg = model(images)[0]
            else:
                buf = torch.empty((len(gv) * B, Cin, Hv, Wv), device=dev, dtype=torch.float32)
                codes = (C.c_int32 * (2 * len(gv)))(*[v for fr in gv for v in fr])
                _lib.call("mgu_tta_views", dev, images, B, Cin, H, W, strides, len(gv), codes, buf)
                lg = model(buf)[0]
            logits.append(lg.permute(0, 2, 3, 1))   # the NHWC storage the forward wrote (contiguous)
        probs = torch.empty((B, H, W, Cls), device=dev, dtype=torch.float32)
        labels = torch.empty((B, H, W), device=dev, dtype=torch.int64)
        conf = torch.empty((B, H, W), device=dev, dtype=torch.float32)
        table = (C.c_int32 * (4 * len(views)))(*[v for row in views for v in row])
        _lib.call("mgu_tta_merge", dev, logits[0], logits[1] if len(logits) > 1 else None, B, Cls, H, W, len(views), table, probs, labels,
                  conf)
    return probs.permute(0, 3, 1, 2), labels, conf


def object_scores(table: ObjectTable, probs: torch.Tensor) -> torch.Tensor:
    """Confidence of every object of `table`: float32 (N,), the mean of probs[b, class_id, y, x] over the object's pixels, in the row
    order of the table's per-object arrays.  probs: float32 (B, C, H, W) on the table's device -- predict_tta's probs (its NHWC
    storage read in place) -- with values in [0, 1] (others are clamped).  Deterministic: fixed-point integer sums, no float atomics."""
    if not isinstance(probs, torch.Tensor) or probs.dim() != 4 or probs.dtype != torch.float32:
        raise TypeError("probs must be (B, C, H, W) float32")
    if not probs.is_cuda or probs.device != table.labels.device:
        raise RuntimeError(f"probs must live on {table.labels.device} (object scores run only on a HIP device)")
    B, Cls, H, W = probs.shape
    if tuple(table.labels.shape) != (B, H, W):
        raise ValueError(f"probs shape {tuple(probs.shape)} does not match the table's labels {tuple(table.labels.shape)}")
    N = table.class_id.numel()
    dev = probs.device
    scores = torch.empty(N, device=dev, dtype=torch.float32)
    if N == 0:
        return scores
    _lib.call("mgu_object_scores", dev, table.labels, nhwc_storage(probs), B, H, W, Cls, table.offsets, N, table.class_id, table.area, scores)
    return scores
