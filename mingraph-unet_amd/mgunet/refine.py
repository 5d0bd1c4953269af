"""Edge-aware refinement on the device: refine_probs filters every class-probability plane with a joint bilateral kernel guided by the
photograph, a fixed number of times, and takes the argmax -- cost-volume filtering (Hosni et al., PAMI 2013), structurally the
message-passing step of a dense CRF.  It sits between "softmax" (predict_tta, predict_tiled, a forward's logits) and
"argmax -> clean_masks -> split_objects", and pulls the outline onto the colour edge of the image, which no other stage reads.

The reference has no such stage: the arithmetic is this build's own (include/mgunet.h states it), in fixed point -- 16-bit
probabilities, integer weights from two host tables, exact uint32 sums -- so the result is bitwise equal to tests/refine_oracle.py and
from run to run.  csrc/refine.hip runs one launch per iteration.  bilateral_tables below is the single host description of the two
tables; the refined planes are NOT renormalised, so they need not sum to 1."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._args import nhwc_storage
from .preprocess import _to_dev_u8
from .tta import MAX_CLASSES

MAX_RADIUS = 7        # csrc/refine.hip RF_MAX_R: 225 taps * 256 * 65535 < 2^32 keeps the uint32 sums exact
MAX_ITERATIONS = 16   # RF_MAX_T
RANGE_ENTRIES = 1024  # RF_RANGE


def bilateral_tables(radius: int, sigma_space: float, sigma_color: float):
    """(space_lut, range_lut, shift) of mgu_refine_probs, computed in float64:
    space_lut int32 (radius + 1, radius + 1), [a][b] = rint(256 exp(-(a^2 + b^2) / (2 sigma_space^2)));
    shift, the smallest s in [0, 8] with ceil(12.5 sigma_color^2) >> s <= 1023 (8 when there is none): the table then reaches squared
    guide distances of 12.5 sigma_color^2, where the Gaussian has fallen to exp(-6.25) -- below half a unit of the 8-bit weight;
    range_lut int32 (1024,), [k] = rint(256 exp(-(k << shift) / (2 sigma_color^2))).
    ValueError for a sigma that is not a positive finite number or a radius outside 1..7."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MAX_RADIUS:
        raise ValueError(f"radius must be an integer in 1..{MAX_RADIUS} (225 taps keep the kernel's uint32 sums exact), got {radius!r}")
    ss, sc = float(sigma_space), float(sigma_color)
    if not (math.isfinite(ss) and ss > 0.0 and math.isfinite(sc) and sc > 0.0):
        raise ValueError(f"sigma_space and sigma_color must be positive and finite, got {sigma_space!r}, {sigma_color!r}")
    r = int(radius)
    a = np.arange(r + 1, dtype=np.float64)
    space = np.rint(256.0 * np.exp(-(a[:, None] ** 2 + a[None, :] ** 2) / (2.0 * ss * ss))).astype(np.int32)
    top = math.ceil(12.5 * sc * sc)
    shift = next((s for s in range(9) if (top >> s) <= RANGE_ENTRIES - 1), 8)
    k = (np.arange(RANGE_ENTRIES, dtype=np.int64) << shift).astype(np.float64)
    rng = np.rint(256.0 * np.exp(-k / (2.0 * sc * sc))).astype(np.int32)
    return space, rng, shift


def _guide_batch(guide, B: int, H: int, W: int, dev) -> torch.Tensor:
    """the guide as a contiguous uint8 (B, H, W, G) tensor on dev"""
    if not isinstance(guide, (np.ndarray, torch.Tensor)):
        raise TypeError("guide must be a uint8 numpy array or tensor")
    if isinstance(guide, torch.Tensor) and guide.is_cuda and guide.device != dev:
        raise RuntimeError(f"guide must live on {dev}")
    g, _ = _to_dev_u8(guide)
    if g.device != dev:
        g = g.to(dev)
    if g.dim() == 2:
        g = g.unsqueeze(-1)
    if g.dim() == 3:
        g = g.unsqueeze(0)
    if g.dim() != 4 or tuple(g.shape[:3]) != (B, H, W) or g.shape[3] not in (1, 3):
        raise ValueError(f"guide shape {tuple(guide.shape)} does not match probabilities {(B, H, W)}: expected uint8 (B, H, W, G), (H, W, G) "
                         "or (H, W) with G 1 or 3")
    return g.contiguous()


def _refine(src, guide, tables, iterations, from_logits, return_changed, who):
    if not isinstance(src, torch.Tensor) or src.dim() != 4 or src.dtype != torch.float32:
        raise TypeError(f"{who}: src must be (B, C, H, W) float32")
    _lib.require_hip(src, who)
    space, rng, shift = tables
    iterations = int(iterations)
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations must lie in 1..{MAX_ITERATIONS}, got {iterations}")
    B, Cls, H, W = src.shape
    if not 1 <= Cls <= MAX_CLASSES:
        raise ValueError(f"{who} supports 1..{MAX_CLASSES} classes, got {Cls}")
    dev = src.device
    g = _guide_batch(guide, B, H, W, dev)
    probs = torch.empty((B, H, W, Cls), device=dev, dtype=torch.float32)
    labels = torch.empty((B, H, W), device=dev, dtype=torch.int64)
    conf = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    changed = torch.zeros((B,), device=dev, dtype=torch.int64) if return_changed else None
    if B * H * W:
        x = nhwc_storage(src)
        sp = np.ascontiguousarray(space, np.int32).reshape(-1)
        rl = np.ascontiguousarray(rng, np.int32).reshape(-1)
        radius = int(round(math.sqrt(sp.size))) - 1
        if (radius + 1) ** 2 != sp.size or rl.size != RANGE_ENTRIES:
            raise ValueError(f"tables of {sp.size} and {rl.size} entries are not (radius + 1)^2 and {RANGE_ENTRIES}")
        _lib.call("mgu_refine_probs", dev, x, 0 if from_logits else 1, g, B, H, W, Cls, g.shape[3], radius,
                  sp.ctypes.data_as(C.c_void_p), rl.ctypes.data_as(C.c_void_p), int(shift), iterations, probs, labels, conf, changed)
    out = (probs.permute(0, 3, 1, 2), labels, conf)
    return out + (changed,) if return_changed else out


def refine_probs(src: torch.Tensor, guide, radius: int = 5, sigma_space: float = 3.0, sigma_color: float = 12.0, iterations: int = 2,
                 from_logits: bool = False, return_changed: bool = False):
    """Class probabilities filtered `iterations` times with a (2 radius + 1)^2 joint bilateral kernel guided by `guide`, then argmax.
    src: float32 (B, C, H, W) on the HIP device, as predict_tta / predict_tiled return it (their NHWC storage is read in place; any
    other layout costs one copy), C <= 16: probabilities (values are clamped to [0, 1], NaN counts as 0), or logits with from_logits
    (each pixel's softmax is taken as predict_tta takes it).  guide: the photograph at the same resolution, uint8 (B, H, W, G),
    (H, W, G) or (H, W), G 1 or 3, a numpy array or a device tensor; the channel order does not matter.
    A tap's weight is the product of a spatial Gaussian (sigma_space, pixels) and a Gaussian of the guide's colour distance
    (sigma_color, grey levels), both 8-bit fixed point (bilateral_tables).  Returns (probs, labels, confidence[, changed]) with
    predict_tta's shapes, dtypes and NHWC storage: probs float32 (B, C, H, W) in steps of 1/65535 and NOT renormalised (the planes need
    not sum to 1), labels int64 (B, H, W) its first maximal class, confidence that class's value; changed int64 (B,) counts the pixels
    whose class differs from the source's.  Bitwise repeatable.  The defaults are API choices, not tuned numbers: pick the radius and
    sigma_color for the images at hand."""
    return _refine(src, guide, bilateral_tables(radius, sigma_space, sigma_color), iterations, from_logits, return_changed, "refine_probs")


class EdgeRefiner:
    """refine_probs with its parameters and tables held: EdgeRefiner(radius, sigma_space, sigma_color, iterations)(src, guide,
    from_logits=False, return_changed=False).  predict_tiled(refine=...) takes one.  The defaults are refine_probs's: API choices, not
    tuned numbers."""

    def __init__(self, radius: int = 5, sigma_space: float = 3.0, sigma_color: float = 12.0, iterations: int = 2):
        self.tables = bilateral_tables(radius, sigma_space, sigma_color)
        iterations = int(iterations)
        if not 1 <= iterations <= MAX_ITERATIONS:
            raise ValueError(f"iterations must lie in 1..{MAX_ITERATIONS}, got {iterations}")
        self.radius, self.sigma_space, self.sigma_color, self.iterations = int(radius), float(sigma_space), float(sigma_color), iterations

    def __call__(self, src: torch.Tensor, guide, from_logits: bool = False, return_changed: bool = False):
        return _refine(src, guide, self.tables, self.iterations, from_logits, return_changed, "EdgeRefiner")

    def __repr__(self):
        return (f"EdgeRefiner(radius={self.radius}, sigma_space={self.sigma_space}, sigma_color={self.sigma_color}, "
                f"iterations={self.iterations})")
