"""The border weight map of the U-Net paper (Ronneberger et al., MICCAI 2015, eq. 2) on the device (csrc/border.hip, INTEGRATION.md
section V): per pixel the exact squared distances to the nearest and to the second-nearest object of an instance map, and

    w(p) = class_weight[cls(p)] + w0 exp(-(d1(p) + d2(p))^2 / (2 sigma^2))

so that the thin background gaps between touching fruits weigh most in losses.pixel_cross_entropy(pixel_weight=).  The instance map
is whatever connected_components / split_objects label (or a dataset's own): int32, 0 = background, every other value an object.
Two launches per call, no host synchronisation, bitwise repeatable."""
from __future__ import annotations

import torch

from . import _lib
from ._args import batched_map
from .objects import ObjectTable

D2_NONE = 1 << 30     # MGU_D2_NONE: no (second) object in the image


def border_options(w0, sigma, num_classes=None, class_weight=None):
    """(w0, sigma) as floats, checked as mgu_border_weights checks them (no device needed): sigma > 0, w0 >= 0, and class weights
    only for up to 8 classes."""
    w0, sigma = float(w0), float(sigma)
    if not sigma > 0.0:
        raise ValueError(f"sigma {sigma!r} must be > 0")
    if not w0 >= 0.0:
        raise ValueError(f"w0 {w0!r} must be >= 0")
    if class_weight is not None:
        if not isinstance(class_weight, torch.Tensor) or class_weight.dim() != 1 or not 1 <= class_weight.numel() <= 8 or \
                (num_classes is not None and class_weight.numel() != num_classes):
            raise ValueError("class_weight must be a tensor of num_classes <= 8 floats")
    return w0, sigma


def _instance_map(labels, who: str) -> torch.Tensor:
    lab = labels.labels if isinstance(labels, ObjectTable) else labels
    if not isinstance(lab, torch.Tensor):
        raise TypeError(f"{who}: labels must be an integer tensor or an ObjectTable")
    lab = batched_map(lab, "an instance map")
    _lib.require_hip(lab, who)
    if lab.numel() == 0:
        raise ValueError(f"{who}: a shape without pixels")
    return lab.to(torch.int32).contiguous()


def _run(lab, classes, class_weight, w0, sigma, background_class, d1sq, d2sq, nearest, weight, target):
    B, H, W = lab.shape
    _lib.call("mgu_border_weights", lab.device, lab, B, H, W, classes, class_weight, 0 if class_weight is None else class_weight.numel(),
              float(w0), float(sigma), int(background_class), d1sq, d2sq, nearest, weight, target)


def border_distances(labels):
    """(d1sq, d2sq, nearest), each int32 (B, H, W), of an integer instance map (H, W) or (B, H, W) or an ObjectTable's labels: the
    exact squared Euclidean distance of every pixel to the nearest object of its image (0 on object pixels), to the second-nearest
    one (the nearest object with another label), and the nearest object's label (equal distances: the smaller label).  2 ** 30 where
    the image has no (second) object, nearest 0 where it has none.  The labels are read as int32."""
    lab = _instance_map(labels, "border_distances")
    out = [torch.empty(lab.shape, device=lab.device, dtype=torch.int32) for _ in range(3)]
    _run(lab, None, None, 0.0, 1.0, 0, out[0], out[1], out[2], None, None)
    return tuple(out)


def border_weights(labels, classes=None, class_weight=None, w0=10.0, sigma=5.0, separate=False, background_class=0):
    """The weight map float32 (B, H, W) of an instance map (see border_distances): class_weight[classes] + w0 exp(-(d1 + d2)^2 /
    (2 sigma^2)), in float64 from the exact distances, rounded once; the defaults are the paper's w0 = 10, sigma = 5 pixels.  classes:
    the int64 class map (B, H, W) the class term is looked up with; a class outside [0, len(class_weight)) (-100) gets class term 0,
    and without classes or class_weight the class term is 1.  separate: also return the training target -- classes with every object
    pixel that has a 4-neighbour of another object set to background_class, the one-pixel gap between touching instances the recipe
    assumes -- as (weights, target)."""
    lab = _instance_map(labels, "border_weights")
    w0, sigma = border_options(w0, sigma, None, class_weight)
    if classes is not None:
        if not isinstance(classes, torch.Tensor) or classes.dtype != torch.int64 or classes.device != lab.device:
            raise TypeError("border_weights: classes must be an int64 tensor on the labels' device")
        classes = batched_map(classes, "a class map")
        if classes.shape != lab.shape:
            raise ValueError(f"border_weights: classes {tuple(classes.shape)} and labels {tuple(lab.shape)} differ in shape")
        classes = classes.contiguous()
    elif separate:
        raise ValueError("border_weights: separate=True needs the class map")
    if class_weight is not None:
        class_weight = class_weight.detach().to(device=lab.device, dtype=torch.float32).contiguous()
    weight = torch.empty(lab.shape, device=lab.device, dtype=torch.float32)
    target = torch.empty(lab.shape, device=lab.device, dtype=torch.int64) if separate else None
    _run(lab, classes, class_weight, w0, sigma, background_class, None, None, None, weight, target)
    return (weight, target) if separate else weight
