"""Host-side mirrors of the reference's auxiliary losses, routed through libmgunet.so: same names,
constructor arguments, call signatures and error messages.  Each call returns a 0-dim float32 tensor on the input's device.
TVLoss, dice_loss, lovasz_softmax, pixel_cross_entropy and FeatureConsistencyLoss are differentiable (torch.autograd.Function nodes whose backward is a HIP kernel:
mgu_*_backward), so `loss.backward()` as at scripts/train_segmentation.py:133 works on them; EllipticalShapeLoss has no gradient
w.r.t. its input (a function of arg-max pixel coordinates; the reference loop pins loss_shape to 0, train_end_to_end.py:287).
check_labels(device) synchronises and raises where F.one_hot would have raised on an out-of-range label.

    TVLoss                   scripts/train_end_to_end.py:73-89
    dice_loss                scripts/train_segmentation.py:29-40
    FeatureConsistencyLoss   model/unet/feature_loss.py:5-125
    EllipticalShapeLoss      model/unet/shape_loss.py:6-180
    lovasz_softmax           the build's own addition (the reference has no IoU surrogate): INTEGRATION.md section Q
    pixel_cross_entropy      the build's own addition (class weights, label smoothing, focal term, hard-pixel mining): section S;
                             with pixel_weight= a per-pixel weight map such as border.border_weights': section V
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach() if t.dtype == torch.float32 else t.detach().float()


def check_labels(device) -> None:
    """Synchronise and raise ValueError if a loss kernel on `device` met a label outside [0, C) since the last check (the place
    F.one_hot raises in the reference, scripts/train_segmentation.py:34); the loss calls themselves never block the host."""
    _lib.call("mgu_loss_sync_check", torch.device(device))


class _TVFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx_, x, weight):
        xd = _f32(x)
        B, C_, H, W = xd.shape
        out = torch.empty((), device=xd.device, dtype=torch.float32)
        _lib.call("mgu_tv_loss", xd.device, xd, B, C_, H, W, *xd.stride(), float(weight), out)
        ctx_.save_for_backward(xd)
        ctx_.weight, ctx_.in_dtype = float(weight), x.dtype
        return out

    @staticmethod
    def backward(ctx_, g):
        (xd,) = ctx_.saved_tensors
        B, C_, H, W = xd.shape
        dx = torch.empty_like(xd)
        g = g.detach().float().contiguous()
        _lib.call("mgu_tv_loss_backward", xd.device, xd, B, C_, H, W, *xd.stride(), ctx_.weight, 1.0, g, dx, *dx.stride())
        return dx.to(ctx_.in_dtype), None


class TVLoss(nn.Module):
    def __init__(self, weight=1.0):
        super().__init__()
        self.weight = weight

    def forward(self, x):
        _lib.require_hip(x, "mgunet TVLoss")
        if x.dim() != 4:
            raise ValueError("expected (B, C, H, W)")
        return _TVFn.apply(x, self.weight)


def _pixel_strided(pd):
    """pd with ONE stride for the pixel index (both NCHW and NHWC storage qualify; anything else is copied)"""
    return pd if pd.stride(2) == pd.shape[3] * pd.stride(3) else pd.contiguous()


def _check_logits(pred, target):
    if pred.dim() != 4 or target.dim() != 3 or target.dtype != torch.int64:
        raise ValueError("expected logits (B, C, H, W) and an int64 target (B, H, W)")


def _logits_head(pred, target):
    """What every entry point of the segmentation losses starts with: (pd, target, head) with pd the float32 pixel-strided logits,
    target contiguous and head = (device, pd, target, B, H * W, C, stride of n, of c, of the pixel index)."""
    pd, target = _pixel_strided(_f32(pred)), target.contiguous()
    B, C_, H, W = pd.shape
    return pd, target, (pd.device, pd, target, B, H * W, C_, pd.stride(0), pd.stride(1), pd.stride(3))


def _grad_args(pd, g):
    """The gradient of the logits pd, with pd's strides (NHWC storage stays NHWC), and the tail every *_backward entry takes before its
    own flags: (grad_scale 1.0, the upstream gradient as contiguous float32, d, d's three strides)."""
    d = torch.empty_strided(pd.shape, pd.stride(), device=pd.device, dtype=torch.float32)
    return d, (1.0, g.detach().float().contiguous(), d, d.stride(0), d.stride(1), d.stride(3))


class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx_, pred, target, smooth):
        pd, target, head = _logits_head(pred, target)
        out = torch.empty((), device=pd.device, dtype=torch.float32)
        _lib.call("mgu_dice_loss", *head, float(smooth), out)
        ctx_.save_for_backward(pd, target)
        ctx_.smooth, ctx_.in_dtype = float(smooth), pred.dtype
        return out

    @staticmethod
    def backward(ctx_, g):
        pd, target, head = _logits_head(*ctx_.saved_tensors)
        d, tail = _grad_args(pd, g)
        _lib.call("mgu_dice_loss_backward", *head, ctx_.smooth, *tail, 0, None)
        return d.to(ctx_.in_dtype), None, None


def dice_loss(pred, target, smooth=1.):
    """pred (B, C, H, W) logits (any strides: NHWC storage is read in place), target (B, H, W) int64.  Differentiable w.r.t. pred.
    A label outside [0, C) -- F.one_hot raises on it -- is reported by check_labels(pred.device) (no host sync inside the call)."""
    _lib.require_hip(pred, "mgunet dice_loss")
    _check_logits(pred, target)
    return _DiceFn.apply(pred, target, smooth)


_LOVASZ_CLASSES = {"present": 0, "all": 1}


class _LovaszFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx_, pred, target, mode, per_image, ignore_index):
        pd, target, head = _logits_head(pred, target)
        out = torch.empty((), device=pd.device, dtype=torch.float32)
        _lib.call("mgu_lovasz_softmax", *head, mode, per_image, ignore_index, out, None, None)
        ctx_.save_for_backward(pd, target)
        ctx_.opts, ctx_.in_dtype = (mode, per_image, ignore_index), pred.dtype
        return out

    @staticmethod
    def backward(ctx_, g):
        pd, target, head = _logits_head(*ctx_.saved_tensors)
        d, tail = _grad_args(pd, g)
        _lib.call("mgu_lovasz_softmax_backward", *head, *ctx_.opts, *tail, 0, None)
        return d.to(ctx_.in_dtype), None, None, None, None


def _lovasz_args(pred, target, classes, per_image, ignore_index):
    _lib.require_hip(pred, "mgunet lovasz_softmax")
    _check_logits(pred, target)
    if classes not in _LOVASZ_CLASSES:
        raise ValueError(f"unknown classes {classes!r}: 'present' or 'all'")
    return _LOVASZ_CLASSES[classes], int(bool(per_image)), int(ignore_index)


def lovasz_softmax(pred, target, classes="present", per_image=False, ignore_index=-100):
    """Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018), the convex surrogate of 1 - IoU: pred
    (B, C, H, W) logits with C <= 8 (any strides dice_loss accepts), target (B, H, W) int64.  classes: "present" averages over the
    classes that occur in the target, "all" over every class; per_image: one loss per image, then their mean; pixels labelled
    ignore_index take no part.  Differentiable w.r.t. pred.  Any other label outside [0, C) makes the loss NaN and is reported by
    check_labels(pred.device) (no host sync inside the call)."""
    return _LovaszFn.apply(pred, target, *_lovasz_args(pred, target, classes, per_image, ignore_index))


def _lovasz_debug(pred, target, classes="present", per_image=False, ignore_index=-100):
    """(loss, errors, ranks) through the test hooks of mgu_lovasz_softmax: errors fp32 and ranks int32, each (C, B, H, W): the
    error of every pixel for every class and its 0-based rank inside its segment (-1: ignored pixel)."""
    mode, per_image, ignore_index = _lovasz_args(pred, target, classes, per_image, ignore_index)
    pd, target, head = _logits_head(pred, target)
    B, C_, H, W = pd.shape
    out = torch.empty((), device=pd.device, dtype=torch.float32)
    errors = torch.empty((C_, B, H, W), device=pd.device, dtype=torch.float32)
    ranks = torch.empty((C_, B, H, W), device=pd.device, dtype=torch.int32)
    _lib.call("mgu_lovasz_softmax", *head, mode, per_image, ignore_index, out, errors, ranks)
    return out, errors, ranks


def pixel_ce_options(weight, label_smoothing, focal_gamma, keep_fraction, min_kept, per_image, num_classes=None):
    """The checked options of the pixel cross-entropy, in the order of the C-ABI after the class weights: (label_smoothing,
    focal_gamma, keep_fraction, min_kept, per_image).  ValueError on what mgu_pixel_ce would refuse, on a weight vector of the
    wrong length (num_classes given) and on a negative weight in a host tensor (weights already on the device are the caller's)."""
    eps, gamma, keep, kmin = float(label_smoothing), float(focal_gamma), float(keep_fraction), int(min_kept)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing {label_smoothing!r} must lie in [0, 1)")
    if not (gamma == 0.0 or gamma >= 1.0):
        raise ValueError(f"focal_gamma {focal_gamma!r} must be 0 or >= 1")
    if gamma > 0.0 and eps > 0.0:
        raise ValueError("focal_gamma > 0 takes no label_smoothing")
    if not 0.0 < keep <= 1.0:
        raise ValueError(f"keep_fraction {keep_fraction!r} must lie in (0, 1]")
    if kmin < 0:
        raise ValueError(f"min_kept {min_kept!r} must be >= 0")
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or weight.dim() != 1 or (num_classes is not None and weight.numel() != num_classes):
            raise ValueError("weight must be a tensor of num_classes floats")
        if weight.device.type == "cpu" and bool((weight.detach() < 0).any()):   # a device tensor is not read back: no host sync
            raise ValueError("class weights must be >= 0")
    return eps, gamma, keep, kmin, int(bool(per_image))


def _pixel_ce_entry(name, head, weight, pixel_weight):
    """The entry point and the arguments up to the options: mgu_pixel_ce[_backward], or with a map mgu_pixel_ce_map[_backward], which
    takes it after the class weights."""
    if pixel_weight is None:
        return (name,) + head + (weight,)
    return (name.replace("mgu_pixel_ce", "mgu_pixel_ce_map"),) + head + (weight, pixel_weight)


class _PixelCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx_, pred, target, weight, opts, ignore_index, pixel_weight=None):
        pd, target, head = _logits_head(pred, target)
        out = torch.empty((), device=pd.device, dtype=torch.float32)
        _lib.call(*_pixel_ce_entry("mgu_pixel_ce", head, weight, pixel_weight), *opts, ignore_index, out, None, None)
        ctx_.save_for_backward(pd, target)
        ctx_.weight, ctx_.opts, ctx_.in_dtype, ctx_.pixel_weight = weight, (opts, ignore_index), pred.dtype, pixel_weight
        return out

    @staticmethod
    def backward(ctx_, g):
        pd, target, head = _logits_head(*ctx_.saved_tensors)
        d, tail = _grad_args(pd, g)
        opts, ignore_index = ctx_.opts
        _lib.call(*_pixel_ce_entry("mgu_pixel_ce_backward", head, ctx_.weight, ctx_.pixel_weight), *opts, ignore_index, *tail, 0, 0, None)
        return d.to(ctx_.in_dtype), None, None, None, None, None   # the map is held fixed: it gets no gradient


def _pixel_ce_args(pred, target, weight, label_smoothing, focal_gamma, keep_fraction, min_kept, per_image, ignore_index):
    _lib.require_hip(pred, "mgunet pixel_cross_entropy")
    _check_logits(pred, target)
    opts = pixel_ce_options(weight, label_smoothing, focal_gamma, keep_fraction, min_kept, per_image, pred.shape[1])
    if weight is not None:
        weight = weight.detach().to(device=pred.device, dtype=torch.float32).contiguous()
    return weight, opts, int(ignore_index)


def pixel_weight_map(pixel_weight, pred):
    """The per-pixel weight map of pixel_cross_entropy as the kernels read it: float32 (B, H, W), dense, on pred's device, detached
    (None stays None).  ValueError on another shape."""
    if pixel_weight is None:
        return None
    B, _, H, W = pred.shape
    if not isinstance(pixel_weight, torch.Tensor) or tuple(pixel_weight.shape) != (B, H, W):
        raise ValueError(f"pixel_weight must be a (B, H, W) = {(B, H, W)} tensor")
    return pixel_weight.detach().to(device=pred.device, dtype=torch.float32).contiguous()


def pixel_cross_entropy(pred, target, weight=None, label_smoothing=0.0, focal_gamma=0.0, keep_fraction=1.0, min_kept=0, per_image=False,
                        ignore_index=-100, pixel_weight=None):
    """Imbalance-aware pixel-wise cross-entropy: pred (B, C, H, W) logits with C <= 8 (any strides
    dice_loss accepts), target (B, H, W) int64.  weight (C floats >= 0) and label_smoothing are nn.CrossEntropyLoss's; focal_gamma
    >= 1 multiplies each pixel's term by (1 - p_y)^gamma (Lin et al. 2017; takes no label_smoothing); keep_fraction < 1 keeps only
    the hardest pixels: of the n counted pixels of the batch (per_image: of each image) the min(n, max(min_kept, ceil(keep_fraction
    n))) with the largest loss, equal losses in pixel order, and only they carry value and gradient.  loss = sum of the kept
    losses / sum of their class weights.  Differentiable w.r.t. pred.  A label outside [0, C) other than ignore_index makes the loss
    NaN and is reported by check_labels(pred.device) (no host sync inside the call).
    pixel_weight: a per-pixel weight map m >= 0 of shape (B, H, W), for example mgunet.border_weights' (INTEGRATION.md section V):
    every pixel's loss becomes m l, that product is what the mining ranks, loss = sum_kept m l / sum_kept m w_y, and m itself gets
    no gradient.  A map of ones gives the bits of the call without one."""
    return _PixelCEFn.apply(pred, target, *_pixel_ce_args(pred, target, weight, label_smoothing, focal_gamma, keep_fraction, min_kept,
                                                          per_image, ignore_index), pixel_weight_map(pixel_weight, pred))


def _pixel_ce_debug(pred, target, weight=None, label_smoothing=0.0, focal_gamma=0.0, keep_fraction=1.0, min_kept=0, per_image=False,
                    ignore_index=-100, pixel_weight=None):
    """(loss, pixel_loss, kept) through the test hooks of mgu_pixel_ce: pixel_loss fp32 (B, H, W), the loss of every pixel (0 where
    it is not counted), and kept int32 (B, H, W): 1 kept, 0 dropped, -1 not counted."""
    weight, opts, ignore_index = _pixel_ce_args(pred, target, weight, label_smoothing, focal_gamma, keep_fraction, min_kept, per_image,
                                                ignore_index)
    pd, target, head = _logits_head(pred, target)
    B, C_, H, W = pd.shape
    out = torch.empty((), device=pd.device, dtype=torch.float32)
    pixel_loss = torch.empty((B, H, W), device=pd.device, dtype=torch.float32)
    kept = torch.empty((B, H, W), device=pd.device, dtype=torch.int32)
    _lib.call(*_pixel_ce_entry("mgu_pixel_ce", head, weight, pixel_weight_map(pixel_weight, pd)), *opts, ignore_index, out, pixel_loss, kept)
    return out, pixel_loss, kept


CLASS_WEIGHT_SCHEMES = ("median_frequency", "inverse", "enet")


def class_weights(counts, scheme="median_frequency"):
    """Class weights from a (C,) vector of pixel counts (for example the row sums of SegmentationEvaluator's confusion matrix), in
    float64 on the host; returns a float32 (C,) tensor.  With f_c = count_c / sum of the counts:
        "median_frequency"  median of the f of the classes that occur / f_c     (Eigen & Fergus, ICCV 2015)
        "inverse"           1 / (number of classes that occur * f_c): the weights of the classes that occur have weighted mean 1
        "enet"              1 / ln(1.02 + f_c)                                  (Paszke et al., ENet, 2016)
    A class with count 0 gets weight 0."""
    if scheme not in CLASS_WEIGHT_SCHEMES:
        raise ValueError(f"unknown scheme {scheme!r}: " + ", ".join(repr(k) for k in CLASS_WEIGHT_SCHEMES[:-1]) +
                         f" or {CLASS_WEIGHT_SCHEMES[-1]!r}")
    n = torch.as_tensor(counts).detach().cpu().to(torch.float64).reshape(-1)
    if n.numel() == 0 or bool((n < 0).any()):
        raise ValueError("counts must be a non-empty vector of non-negative numbers")
    seen = n > 0
    w = torch.zeros_like(n)
    if bool(seen.any()):
        f = n[seen] / n.sum()
        if scheme == "median_frequency":
            w[seen] = f.sort().values[(f.numel() - 1) // 2:f.numel() // 2 + 1].mean() / f
        elif scheme == "inverse":
            w[seen] = 1.0 / (f.numel() * f)
        else:
            w[seen] = 1.0 / torch.log(1.02 + f)
    return w.to(torch.float32)


class _FeatConsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx_, f_unet, f_graph, y, margin):
        fu, fg = _f32(f_unet).contiguous(), _f32(f_graph).contiguous()
        B, N, D = fu.shape
        out = torch.empty((), device=fu.device, dtype=torch.float32)
        _lib.call("mgu_feature_consistency_loss", fu.device, fu, fg, y, B, N, D, float(margin), out)
        ctx_.save_for_backward(fu, fg, y)
        ctx_.margin = float(margin)
        return out

    @staticmethod
    def backward(ctx_, g):
        fu, fg, y = ctx_.saved_tensors
        B, N, D = fu.shape
        need_u, need_g = ctx_.needs_input_grad[0], ctx_.needs_input_grad[1]
        du = torch.empty_like(fu) if need_u else None
        dg = torch.empty_like(fg) if need_g else None
        g = g.detach().float().contiguous()
        _lib.call("mgu_feature_consistency_loss_backward", fu.device, fu, fg, y, B, N, D, ctx_.margin, 1.0, g, du, dg)
        return du, dg, None, None


class FeatureConsistencyLoss(nn.Module):
    def __init__(self, margin=1.0):
        super().__init__()
        self.margin = margin

    def forward(self, f_unet, f_graph, correspondence_map_y, regions_unet=None, regions_graph=None):
        _lib.require_hip(f_unet, "mgunet FeatureConsistencyLoss")
        B, N, D = f_unet.shape                                                  # (N, D) inputs raise here, as in the reference (:88)
        if f_unet.shape != f_graph.shape:
            raise ValueError(f"f_unet ({f_unet.shape}) and f_graph ({f_graph.shape}) must have same dimensions for this loss version.")
        if correspondence_map_y.shape != (B, N):
            raise ValueError(f"correspondence_map_y (patch_region_labels_y) shape ({correspondence_map_y.shape}) "
                             f"is not (Batch, Num_Patches) = ({B}, {N}).")
        if D % 4:
            raise ValueError("the feature width must be a multiple of 4 (16-byte lanes)")
        return _FeatConsFn.apply(f_unet, f_graph, correspondence_map_y.detach().float().contiguous(), self.margin)


class EllipticalShapeLoss(nn.Module):
    def __init__(self, epsilon=1e-6):
        super().__init__()
        self.epsilon = epsilon

    def forward(self, segmentation_probs, object_masks_list=None, objects=None):
        """The reference's two forms (object_masks_list given, or the whole class-1 foreground of each image as ONE object), plus
        the per-instance form the reference asks for (shape_loss.py:42-48, :85-92) through `objects`: an ObjectTable runs the loss
        over that table's objects; True labels the arg-max map of segmentation_probs (B, C, H, W) float32 with 8-connectivity and
        background 0 (:86-91), keeps the objects of class 1 (:68) and runs the loss per instance.  Both use
        mgunet.object_shapes: one pass over the label map, no dense masks.  Note that the reference's term is about 7/3 for a
        perfect ellipse, not 0: see ObjectShapes."""
        if objects is not None and objects is not False:
            if object_masks_list is not None:
                raise ValueError("pass object_masks_list or objects, not both")
            from .objects import connected_components, object_shapes
            if objects is True:
                _lib.require_hip(segmentation_probs, "mgunet EllipticalShapeLoss")
                if segmentation_probs.dim() != 4:
                    raise ValueError("expected probabilities (B, C, H, W)")
                if segmentation_probs.shape[1] <= 1:       # no foreground class (:63-70)
                    return torch.tensor(0.0, device=segmentation_probs.device)
                table = connected_components(_f32(segmentation_probs), connectivity=2, background=0)
                return object_shapes(table, epsilon=self.epsilon).loss(keep_class=1)
            return object_shapes(objects, epsilon=self.epsilon).loss()
        if object_masks_list is None:
            _lib.require_hip(segmentation_probs, "mgunet EllipticalShapeLoss")
            p = _f32(segmentation_probs)
            B, C_, H, W = p.shape
            if p.stride(2) != W * p.stride(3):
                p = p.contiguous()
            out = torch.empty((), device=p.device, dtype=torch.float32)
            _lib.call("mgu_elliptical_shape_loss_probs", p.device, p, B, C_, H, W, p.stride(0), p.stride(1), p.stride(3), float(self.epsilon),
                      out)
            return out
        masks = [m for img in object_masks_list for m in img]
        if not masks:
            dev = segmentation_probs.device if segmentation_probs is not None else torch.device("cuda")
            return torch.tensor(0.0, device=dev)
        _lib.require_hip(masks[0], "mgunet EllipticalShapeLoss")
        stack = torch.stack([(m != 0) for m in masks]).to(torch.uint8).contiguous()   # (M, H, W): one pass over all objects
        M, H, W = stack.shape
        out = torch.empty((), device=stack.device, dtype=torch.float32)
        _lib.call("mgu_elliptical_shape_loss_masks", stack.device, stack, M, H, W, float(self.epsilon), out)
        return out
