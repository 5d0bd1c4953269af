"""Tiled inference on the device: predict_tiled runs a UNet over an image of any size as overlapping tiles of the size the network was
trained at and blends their softmax probabilities into one full-resolution canvas, which feeds connected_components, object_scores
and object_shapes unchanged.

Per chunk of tiles_per_batch tiles, csrc/tiled.hip writes the tiles as one contiguous batch (one launch, reflect-101 padded where the
image is smaller than the tile; from uint8 the normalisation is applied on the way), the model runs one forward on it, and one launch
adds the chunk's windowed softmaxes to the canvas.  tile_grid and tile_weights below are the single host description of the grid and
the window: the kernels apply the same grid rule and read the weight tables, and tests/tiled_oracle.py restates them in numpy."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .preprocess import _to_dev_u8
from .refine import EdgeRefiner
from .tta import MAX_CLASSES, TRANSFORMS, predict_tta
from .unet import UNet

WINDOWS = ("ramp", "flat")
DEFAULT_MEAN, DEFAULT_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # ImagePreprocessor's


def _axis_origins(L: int, T: int, o: int) -> list:
    if L <= T:
        return [0]
    S = T - o
    n = -(-(L - T) // S) + 1
    return [k * S for k in range(n - 1)] + [L - T]


def _pair(v, what):
    a, b = (v, v) if isinstance(v, (int, np.integer)) else tuple(v)
    a, b = int(a), int(b)
    if a < 1 or b < 1:
        raise ValueError(f"{what} must be positive, got {v!r}")
    return a, b


def tile_grid(H: int, W: int, tile, overlap: int):
    """(origins_y, origins_x): per axis, for image length L, tile T and stride S = T - overlap, [0] when L <= T, otherwise
    ceil((L - T) / S) + 1 origins k * S with the last moved back to L - T.  tile: an int or (Th, Tw).  The 2-D grid is the product of
    the two lists; tile t of an image is (row, col) = divmod(t, len(origins_x))."""
    Th, Tw = _pair(tile, "tile")
    H, W, overlap = int(H), int(W), int(overlap)
    if H < 1 or W < 1:
        raise ValueError(f"image size must be positive, got {(H, W)}")
    if overlap < 0 or overlap >= min(Th, Tw):
        raise ValueError(f"overlap must lie in [0, tile): overlap {overlap}, tile {(Th, Tw)}")
    return _axis_origins(H, Th, overlap), _axis_origins(W, Tw, overlap)


def tile_weights(L: int, T: int, overlap: int, origins, window: str = "ramp") -> np.ndarray:
    """float32 (n, T): row k, entry i = w(i) / (sum of w(p - origin_k') over the tiles k' covering image coordinate p = origins[k] + i).
    "ramp": w(i) = min(1, (i + 1) / (o + 1), (T - i) / (o + 1)); "flat": w(i) = 1.  The window is kept as the integer
    min(o + 1, i + 1, T - i) until one float64 division, so a coordinate under one tile gets exactly 1.0 and a regular ramp seam
    exactly (i + 1) / (o + 1); the result is rounded to float32 once.  Entries past the image (L < T) are never read."""
    if window not in WINDOWS:
        raise ValueError(f"unknown window {window!r}; expected one of {list(WINDOWS)}")
    L, T, o = int(L), int(T), int(overlap)
    if o < 0 or o >= T:
        raise ValueError(f"overlap must lie in [0, tile): overlap {o}, tile {T}")
    i = np.arange(T, dtype=np.int64)
    w = np.minimum(o + 1, np.minimum(i + 1, T - i)) if window == "ramp" else np.ones(T, np.int64)
    span = max(L, T)
    total = np.zeros(span, np.int64)
    for org in origins:
        total[org:org + T] += w
    out = np.empty((len(origins), T), np.float64)
    for k, org in enumerate(origins):
        out[k] = w / total[org:org + T]
    return out.astype(np.float32)


class TilePlan:
    """The grid of a (B, H, W) batch with its weight tables on the device, and the three launches of csrc/tiled.hip on it."""

    def __init__(self, B: int, H: int, W: int, tile, overlap: int, window: str, device):
        self.B, self.H, self.W, self.overlap = int(B), int(H), int(W), int(overlap)
        self.Th, self.Tw = _pair(tile, "tile")
        self.origins_y, self.origins_x = tile_grid(H, W, (self.Th, self.Tw), overlap)
        self.nrows, self.ncols = len(self.origins_y), len(self.origins_x)
        self.ntiles = self.B * self.nrows * self.ncols
        self.device = device
        wy = tile_weights(H, self.Th, overlap, self.origins_y, window)
        wx = tile_weights(W, self.Tw, overlap, self.origins_x, window)
        self.wy, self.wx = torch.from_numpy(wy).to(device), torch.from_numpy(wx).to(device)

    def _grid_args(self):
        return (self.Th, self.Tw, self.overlap, self.overlap)

    def gather(self, images: torch.Tensor, t0: int, n: int, out: torch.Tensor = None) -> torch.Tensor:
        """tiles [t0, t0 + n) of float32 (B, Cin, H, W) `images` (any strides) -> contiguous (n, Cin, Th, Tw)"""
        Cin = images.shape[1]
        if out is None:
            out = torch.empty((n, Cin, self.Th, self.Tw), device=self.device, dtype=torch.float32)
        strides = (C.c_int64 * 4)(*images.stride())
        _lib.call("mgu_tile_gather", self.device, images, self.B, Cin, self.H, self.W, strides, *self._grid_args(), t0, n, out)
        return out

    def gather_u8(self, images: torch.Tensor, bgr: bool, mean, std, t0: int, n: int, out: torch.Tensor = None) -> torch.Tensor:
        """tiles [t0, t0 + n) of contiguous uint8 (B, H, W, 3) `images`, normalised -> contiguous float32 (n, 3, Th, Tw)"""
        if out is None:
            out = torch.empty((n, 3, self.Th, self.Tw), device=self.device, dtype=torch.float32)
        m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        _lib.call("mgu_tile_gather_u8", self.device, images, self.B, self.H, self.W, int(bool(bgr)), m3, s3, *self._grid_args(), t0, n, out)
        return out

    def accumulate(self, tiles: torch.Tensor, t0: int, canvas: torch.Tensor, labels: torch.Tensor = None, conf: torch.Tensor = None,
                   is_prob: bool = False) -> None:
        """adds the chunk `tiles`, contiguous float32 NHWC (n, Th, Tw, C) holding tiles [t0, t0 + n), to the NHWC `canvas`"""
        n, Cls = tiles.shape[0], tiles.shape[3]
        if tuple(tiles.shape[1:3]) != (self.Th, self.Tw) or tiles.dtype != torch.float32 or not tiles.is_contiguous():
            raise ValueError(f"the chunk must be contiguous float32 NHWC (n, {self.Th}, {self.Tw}, C), got {tuple(tiles.shape)} {tiles.dtype}")
        if tuple(canvas.shape) != (self.B, self.H, self.W, Cls) or canvas.dtype != torch.float32 or not canvas.is_contiguous():
            raise ValueError(f"the canvas must be contiguous float32 NHWC ({self.B}, {self.H}, {self.W}, {Cls})")
        _lib.call("mgu_tile_accumulate", self.device, tiles, int(bool(is_prob)), self.B, Cls, self.H, self.W, *self._grid_args(), self.wy,
                  self.wx, t0, n, canvas, labels, conf)

    def finish(self, canvas: torch.Tensor, labels: torch.Tensor, conf: torch.Tensor) -> None:
        _lib.call("mgu_tile_finish", self.device, canvas, self.B, canvas.shape[3], self.H, self.W, labels, conf)


def predict_tiled(model: UNet, images, tile=512, overlap: int = 64, window: str = "ramp", transforms: str = "none",
                  tiles_per_batch: int = 8, mean=None, std=None, bgr: bool = False, refine: EdgeRefiner = None, guide=None):
    """Softmax probabilities of `model` over images of any size: the network runs on overlapping `tile`-sized crops (tile_grid),
    tiles_per_batch of them per forward, and every pixel gets the window-weighted mean (tile_weights) of the softmaxes of the tiles that
    cover it, added in tile order -- bitwise repeatable and independent of tiles_per_batch given the same tile logits.
    images: float32 (B, Cin, H, W) on the HIP device, any strides; or uint8 (H, W, 3) / (B, H, W, 3), a numpy array or a device
    tensor, normalised on the way with mean / std (default: ImagePreprocessor's) and read as BGR when `bgr`, so that a tile is bitwise
    the crop of ImagePreprocessor's output at native size.  An image smaller than the tile is reflect-padded; the padding is computed
    but never written.  transforms != "none": each chunk goes through predict_tta and its averaged probabilities are blended.
    refine: an EdgeRefiner; the blended canvas then goes through it (mgunet.refine) before the return, guided by `guide` -- uint8
    (B, H, W, G), (H, W, G) or (H, W) -- which defaults to uint8 `images` themselves (bgr does not matter to a colour distance) and is
    required with float32 images.  Without `refine` nothing changes, and a `guide` is an error.
    Returns (probs, labels, confidence) with predict_tta's shapes, dtypes and NHWC storage."""
    if not isinstance(model, UNet):
        raise TypeError(f"predict_tiled needs an mgunet.UNet, got {type(model).__name__}")
    if model.training:
        raise RuntimeError("tiled inference is an inference mode: call .eval() first")
    if transforms not in TRANSFORMS:
        raise ValueError(f"unknown transforms {transforms!r}; expected one of {sorted(TRANSFORMS)}")
    if window not in WINDOWS:
        raise ValueError(f"unknown window {window!r}; expected one of {list(WINDOWS)}")
    if refine is not None and not isinstance(refine, EdgeRefiner):
        raise TypeError(f"refine must be an mgunet.EdgeRefiner, got {type(refine).__name__}")
    if refine is None and guide is not None:
        raise ValueError("guide applies only with refine=EdgeRefiner(...)")
    Th, Tw = _pair(tile, "tile")
    overlap, per = int(overlap), int(tiles_per_batch)
    if overlap < 0 or overlap >= min(Th, Tw):
        raise ValueError(f"overlap must lie in [0, tile): overlap {overlap}, tile {(Th, Tw)}")
    if min(Th, Tw) < 2 ** model.depth:
        raise ValueError(f"a {(Th, Tw)} tile is smaller than 2**depth = {2 ** model.depth}, the least the network can pool")
    if per < 1:
        raise ValueError("tiles_per_batch must be at least 1")
    Cls = model.num_classes
    if Cls > MAX_CLASSES:
        raise ValueError(f"predict_tiled supports at most {MAX_CLASSES} classes, the model has {Cls}")
    u8 = isinstance(images, np.ndarray) or (isinstance(images, torch.Tensor) and images.dtype == torch.uint8)
    if u8:
        if images.ndim not in (3, 4) or images.shape[-1] != 3:
            raise ValueError("expected a uint8 (H, W, 3) or (B, H, W, 3) image")
        images, _ = _to_dev_u8(images)
        if images.dim() == 3:
            images = images.unsqueeze(0)
        B, H, W, Cin = images.shape
        mean, std = tuple(mean if mean is not None else DEFAULT_MEAN), tuple(std if std is not None else DEFAULT_STD)
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std must have 3 entries")
    else:
        if not isinstance(images, torch.Tensor) or images.dim() != 4:
            raise ValueError("expected a (B,C,H,W) float32 tensor or a uint8 (H,W,3) / (B,H,W,3) image")
        _lib.require_hip(images, "predict_tiled")
        if images.dtype != torch.float32:
            raise TypeError(f"expected float32 or uint8 input, got {images.dtype}")
        if mean is not None or std is not None or bgr:
            raise ValueError("mean, std and bgr apply to uint8 images only; a float32 batch is taken as already normalised")
        B, Cin, H, W = images.shape
        if refine is not None and guide is None:
            raise ValueError("refine with float32 images needs a uint8 guide: the normalised batch is no photograph")
    if Cin != model.in_channels:
        raise RuntimeError(f"expected {model.in_channels} input channels, got {Cin}")
    if B == 0 or H == 0 or W == 0:
        raise ValueError("predict_tiled needs a non-empty batch")
    dev = images.device
    plan = TilePlan(B, H, W, (Th, Tw), overlap, window, dev)
    probs = torch.empty((B, H, W, Cls), device=dev, dtype=torch.float32)   # every pixel is written by its first covering tile
    labels = torch.empty((B, H, W), device=dev, dtype=torch.int64)
    conf = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    with torch.no_grad():
        for t0 in range(0, plan.ntiles, per):
            n = min(per, plan.ntiles - t0)
            buf = plan.gather_u8(images, bgr, mean, std, t0, n) if u8 else plan.gather(images, t0, n)
            if transforms == "none":
                out, is_prob = model(buf)[0], False
            else:
                out, is_prob = predict_tta(model, buf, transforms)[0], True
            plan.accumulate(out.permute(0, 2, 3, 1), t0, probs, labels, conf, is_prob=is_prob)   # the NHWC storage, contiguous
    if refine is not None:
        return refine(probs.permute(0, 3, 1, 2), images if guide is None else guide)
    return probs.permute(0, 3, 1, 2), labels, conf
