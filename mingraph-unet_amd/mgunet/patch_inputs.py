"""The graph branch's inputs for a whole batch, on the device:

    patch_node_features      scripts/graph_refinement.py:72-113   (patch pixel mean x 16 | Sobel mean | equalised-image means
                                                                   [| smoothed-image means])
    patch_labels             scripts/train_end_to_end.py:340      ("argmax of initial_seg_logits_single, pooled over patch regions")

The training script draws both from torch's RNG (train_end_to_end.py:326, :342).  patch_node_features replaces the per-image
composition patch_features_u8(EdgeDetector().sobel_edges(img), p) / patch_features_u8(HistogramEqualizer().equalize_histogram_rgb(img),
p, True) / torch.cat -- about nine launches per image, two full maps through HBM -- with three launches for the batch and no map, and
gives the same bytes' means bit for bit.  patch_labels is one launch.  E2ETrainer.step_images feeds both to E2ETrainer.step."""
from __future__ import annotations

import torch

from . import _lib
from ._args import nhwc_storage
from .preprocess import CLAHE, _to_dev_u8, patch_clahe_features_u8, patch_smooth_features_u8

MAX_CLASSES = 32   # mgu_patch_labels: lane c of a wave counts class c


def _grid(H: int, W: int, p: int):
    if p < 1:
        raise ValueError(f"patch_size must be positive, got {p}")
    return (H + p - 1) // p, (W + p - 1) // p


def _used_columns(repeat, unet_cols, per_channel, with_images, smooth=False) -> int:
    return (int(repeat) if with_images else 0) + int(unet_cols) + 1 + (3 if per_channel else 1) * (2 if smooth else 1)


def feature_width(repeat: int = 16, unet_cols: int = 0, per_channel: bool = True, pad_to: int = 4, with_images: bool = True,
                  smooth: bool = False) -> int:
    """Row width patch_node_features returns: the used columns (with the smoothed-image block when smooth) rounded up to a multiple of
    pad_to."""
    used = _used_columns(repeat, unet_cols, per_channel, with_images, smooth)
    pad_to = max(1, int(pad_to))
    return (used + pad_to - 1) // pad_to * pad_to


def patch_node_features(images_u8, patch_size: int, images: torch.Tensor = None, repeat: int = 16, unet_patch_feats: torch.Tensor = None,
                        per_channel: bool = True, pad_to: int = 4, out: torch.Tensor = None, smoother=None, equalizer=None) -> torch.Tensor:
    """images_u8: (H, W, 3) or (B, H, W, 3) RGB uint8, numpy or tensor -> (B*Np, F) float32 rows on the device, image b's patches at rows
    [b*Np, (b+1)*Np) in raster order (zero padded bottom / right, as image_to_patches).  Columns: the mean of the normalised float
    batch `images` (B, 3, H, W) -- NCHW or the U-Net's NHWC-storage view, read by strides, no copy -- over the patch and its channels,
    repeated `repeat` times (none without `images`); `unet_patch_feats` (B*Np, Cu) copied (e.g. the rows mgu_unet_request_patch_mean
    wrote); the mean Sobel byte; the mean equalised bytes per channel (or over all three); zeros up to F = the used columns rounded up
    to a multiple of pad_to (the GAT wants Fin % 4 == 0).  With `smoother` (a GaussianSmoother) the "Smooth" block of
    graph_refinement.py:81 follows the equalised columns: the mean bytes of smoother.smooth(image b), per channel or over all three as
    per_channel says -- one more launch, no smoothed image written; without it the output and the launches are unchanged.  With
    `equalizer` (a CLAHE) the equalised columns hold the mean bytes of equalizer.apply(image b) instead of the globally equalised image's
    -- two more launches after the call that fills the row, no equalised image written; the row width and every other column stay as
    they are, and equalizer=None makes exactly the calls and the bytes it made before."""
    if equalizer is not None and not isinstance(equalizer, CLAHE):
        raise TypeError("equalizer must be a CLAHE instance or None")
    if images is not None:
        if not isinstance(images, torch.Tensor) or images.dtype != torch.float32:
            raise TypeError("images must be a float32 (B, 3, H, W) tensor")
        _lib.require_hip(images, "mgunet.patch_node_features")
    if unet_patch_feats is not None:
        _lib.require_hip(unet_patch_feats, "mgunet.patch_node_features")
    u8, _ = _to_dev_u8(images_u8)
    if u8.dim() == 3:
        u8 = u8.unsqueeze(0)
    if u8.dim() != 4 or u8.shape[3] != 3:
        raise ValueError("Input image must be an RGB image (H, W, 3) or a batch (B, H, W, 3).")
    B, H, W, _c = u8.shape
    p = int(patch_size)
    nph, npw = _grid(H, W, p)
    rows = B * nph * npw
    dev = u8.device
    strides = (0, 0, 0, 0)
    if images is not None:
        if images.dim() == 3:
            images = images.unsqueeze(0)
        if tuple(images.shape) != (B, 3, H, W) or images.device != dev:
            raise ValueError(f"images must be ({B}, 3, {H}, {W}) on the device of images_u8, got {tuple(images.shape)} on {images.device}")
        strides = tuple(images.stride())
    cu = 0
    if unet_patch_feats is not None:
        f = unet_patch_feats
        if f.dtype != torch.float32 or f.device != dev or f.numel() == 0 or f.numel() % rows:
            raise ValueError(f"unet_patch_feats must be float32 ({rows}, Cu) rows on the device of images_u8")
        unet_patch_feats = f.reshape(rows, -1).contiguous()
        cu = unet_patch_feats.shape[1]
    F = feature_width(repeat, cu, per_channel, pad_to, images is not None, smoother is not None)
    if out is None:
        out = torch.empty((rows, F), device=dev, dtype=torch.float32)
    elif tuple(out.shape) != (rows, F) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"`out` must be a contiguous float32 ({rows}, {F}) tensor on the images' device")
    _lib.call("mgu_patch_node_features_u8", dev, u8, B, H, W, p, images, *strides, int(repeat) if images is not None else 0,
              unet_patch_feats, cu, 1 if per_channel else 0, out, F)
    if equalizer is not None:    # over the equalised block the call above wrote
        patch_clahe_features_u8(u8, p, equalizer, per_channel, out=out, col0=(int(repeat) if images is not None else 0) + cu + 1)
    if smoother is not None:     # after the call above, which zeroes every column past its own
        patch_smooth_features_u8(u8, p, smoother, per_channel, out=out, col0=_used_columns(repeat, cu, per_channel, images is not None))
    return out


def patch_labels(src: torch.Tensor, patch_size: int, num_classes: int = None, return_counts: bool = False, return_purity: bool = False):
    """One class per patch: the most frequent class among the patch's real pixels, the lowest class on ties.  src: an integer (B, H, W) /
    (H, W) class map on the device (values outside [0, num_classes), e.g. -100, are counted nowhere; num_classes=None takes max + 1,
    which reads the maximum back), or float (B, C, H, W) logits, whose per-pixel class is argmax_classes' -- the U-Net's NHWC-storage
    view is used in place, a contiguous NCHW tensor is permuted once.  -> (B, Np) int64 labels [, (B, Np, C) int32 counts]
    [, (B, Np) float32 purity = majority count / real pixels]; a patch with no counted pixel has label 0 and purity 0."""
    if not isinstance(src, torch.Tensor):
        raise TypeError("src must be a device tensor: an integer class map or float logits")
    _lib.require_hip(src, "mgunet.patch_labels")
    p = int(patch_size)
    if src.is_floating_point():
        if src.dim() != 4:
            raise ValueError("logits must be (B, C, H, W)")
        B, C, H, W = src.shape
        if num_classes is not None and int(num_classes) != C:
            raise ValueError(f"num_classes {num_classes} but the logits have {C} channels")
        data = nhwc_storage(src.float())
        kind = 1
    else:
        if src.dim() == 2:
            src = src.unsqueeze(0)
        if src.dim() != 3:
            raise ValueError("a class map must be (B, H, W) or (H, W)")
        B, H, W = src.shape
        data = src.to(torch.int64).contiguous()
        C = int(num_classes) if num_classes is not None else max(1, int(data.max().item()) + 1)
        kind = 0
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"patch_labels: {C} classes (1..{MAX_CLASSES})")
    nph, npw = _grid(H, W, p)
    Np = nph * npw
    labels = torch.empty((B, Np), device=src.device, dtype=torch.int64)
    counts = torch.empty((B, Np, C), device=src.device, dtype=torch.int32) if return_counts else None
    purity = torch.empty((B, Np), device=src.device, dtype=torch.float32) if return_purity else None
    _lib.call("mgu_patch_labels", src.device, data, kind, B, H, W, C, p, counts, labels, purity)
    res = (labels,) + ((counts,) if return_counts else ()) + ((purity,) if return_purity else ())
    return res if len(res) > 1 else labels
