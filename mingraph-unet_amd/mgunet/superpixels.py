"""Superpixel graphs on the device: per image of a uint8 batch an over-segmentation (integer SLIC, gSLIC formulation), its region
adjacency graph as a CSR with border lengths, a node-feature table and the means of feature maps over the regions -- the producer of
the graphs GATNetwork / gat_forward_csr and FeatureFusion(region_to_pixel_map=) accept beyond the regular patch grid.

The reference has no such stage (its region graph is a fully connected placeholder, its GraphPartitionerUtil an empty stub): the
arithmetic is this build's own (include/mgunet.h states it), integers throughout, so every output is bitwise
equal to tests/superpixels_oracle.py and from run to run.  csrc/superpixels.hip runs a fixed number of launches per stage and never
synchronises with the host.  lab_tables() below is the single host description of the three colour tables."""
from __future__ import annotations

import ctypes as C
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._args import nhwc_storage
from .preprocess import _to_dev_u8

MIN_STEP, MAX_STEP = 4, 128     # csrc/superpixels.hip: a 32 x 32 tile meets at most 11 x 11 centres; int32 sums hold 9 * 128^2 pixels
MAX_MQ = 1024
MAX_ITERATIONS = 32
MAX_ROUNDS = 8
FEATURE_WIDTH = 8


@functools.lru_cache(maxsize=None)
def _lab_tables():
    v = np.arange(256, dtype=np.float64) / 255.0
    lin = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    LIN = np.rint(4095.0 * lin).astype(np.uint16)
    xyz = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]], np.float64)
    M = np.rint(4096.0 * xyz / xyz.sum(axis=1, keepdims=True)).astype(np.int32)
    for r in range(3):
        M[r, int(np.argmax(M[r]))] += 4096 - int(M[r].sum())
    t = np.arange(4096, dtype=np.float64) / 4095.0
    d = 6.0 / 29.0
    f = np.where(t > d ** 3, np.cbrt(t), t / (3.0 * d * d) + 4.0 / 29.0)
    F = np.rint(1024.0 * f).astype(np.uint16)
    for a in (LIN, M, F):
        a.setflags(write=False)
    return LIN, M, F


def lab_tables():
    """(LIN, M, F), computed in float64: the fixed-point CIELAB of mgu_slic_labels / mgu_regions_features_u8, in quarter Lab units.
    LIN uint16 (256,) = rint(4095 srgb_to_linear(v / 255)); M int32 (3, 3) = rint(4096 row) of the sRGB -> XYZ (D65) matrix with each
    row divided by its sum (the white point folded in), the largest coefficient of a row adjusted so the row sums to exactly 4096;
    F uint16 (4096,) = rint(1024 f(t / 4095)) with the CIELAB f (141..1024).  Per pixel xyz_c = (M_c . lin + 2048) >> 12,
    L = (116 F[y] - 16384 + 128) >> 8, a = (500 (F[x] - F[y]) + 128) >> 8, b = (200 (F[y] - F[z]) + 128) >> 8 (arithmetic shifts).
    The arrays are read-only and shared."""
    return _lab_tables()


def _table_args():
    LIN, M, F = lab_tables()
    return LIN.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p), F.ctypes.data_as(C.c_void_p)


def _images(images, who: str) -> torch.Tensor:
    """the photographs as a contiguous uint8 (B, H, W, 3) device tensor; (H, W, 3) is a batch of one"""
    if isinstance(images, torch.Tensor) and images.dtype == torch.uint8:
        _lib.require_hip(images, who)
    img, _ = _to_dev_u8(images)
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[3] != 3:
        raise ValueError(f"{who}: expected uint8 (B, H, W, 3) or (H, W, 3) images, got {tuple(img.shape)}")
    return img.contiguous()


def _step(H: int, W: int, step, n_segments) -> int:
    if (step is None) == (n_segments is None):
        raise ValueError("give exactly one of step and n_segments")
    if step is None:
        if int(n_segments) < 1:
            raise ValueError(f"n_segments must be >= 1, got {n_segments}")
        step = max(MIN_STEP, int(math.sqrt(H * W / int(n_segments)) + 0.5))
    step = int(step)
    if not MIN_STEP <= step <= MAX_STEP:
        raise ValueError(f"the grid step must lie in {MIN_STEP}..{MAX_STEP}, got {step}")
    return step


def _labels(labels: torch.Tensor, offsets: torch.Tensor, who: str):
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int32 or labels.dim() != 3:
        raise TypeError(f"{who}: labels must be an int32 (B, H, W) tensor")
    _lib.require_hip(labels, who)
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.numel() != labels.shape[0] + 1 or \
            offsets.device != labels.device:
        raise TypeError(f"{who}: offsets must be an int64 (B + 1) tensor on the labels' device")
    return labels.contiguous(), offsets.contiguous()


def slic_labels(images_u8, step: int = None, n_segments: int = None, compactness: float = 10.0, iterations: int = 10,
                return_centres: bool = False):
    """Integer SLIC of a uint8 batch (B, H, W, 3) or (H, W, 3), numpy or device tensor -> raw labels int32 (B, H, W) in [0, gx gy),
    gx = ceil(W / step), gy = ceil(H / step).  Exactly one of step (4..128) and n_segments (step = max(4, int(sqrt(H W / n_segments)
    + 0.5))) is given; compactness m in Lab units enters as mq = round(4 m) in 1..1024; `iterations` assignment passes (1..32) with
    iterations - 1 centre updates in between.  return_centres: also int32 (B, gx gy, 6) [x, y, L, a, b, n] as the last pass read them.
    Raw labels need not be connected: connect_regions makes regions of them.  2 iterations + 1 launches, no host synchronisation."""
    if not isinstance(images_u8, (np.ndarray, torch.Tensor)):
        raise TypeError("slic_labels: images must be a uint8 numpy array or tensor")
    shape = images_u8.shape
    if len(shape) not in (3, 4):
        raise ValueError(f"slic_labels: expected uint8 (B, H, W, 3) or (H, W, 3) images, got {tuple(shape)}")
    H, W = (shape[0], shape[1]) if len(shape) == 3 else (shape[1], shape[2])
    S = _step(H, W, step, n_segments)
    mq = int(round(4.0 * float(compactness)))
    if not 1 <= mq <= MAX_MQ:
        raise ValueError(f"compactness {compactness!r} gives mq = round(4 m) = {mq}, outside 1..{MAX_MQ}")
    T = int(iterations)
    if not 1 <= T <= MAX_ITERATIONS:
        raise ValueError(f"iterations must lie in 1..{MAX_ITERATIONS}, got {iterations}")
    img = _images(images_u8, "slic_labels")
    B = img.shape[0]
    gx, gy = -(-W // S), -(-H // S)
    raw = torch.empty((B, H, W), device=img.device, dtype=torch.int32)
    centres = torch.empty((B, gx * gy, 6), device=img.device, dtype=torch.int32) if return_centres else None
    _lib.call("mgu_slic_labels", img.device, img, B, H, W, S, mq, T, *_table_args(), raw, centres)
    return (raw, centres) if return_centres else raw


def connect_regions(raw: torch.Tensor, min_area: int, rounds: int = 2):
    """Raw labels int32 (B, H, W) -> (labels int32 (B, H, W), counts int64 (B), offsets int64 (B + 1)): the 4-connected same-value
    components, then `rounds` (0..8) merge rounds in which every region of area < min_area joins the 4-adjacent region of area >=
    min_area it shares the most pixel edges with (ties: the one whose first pixel comes first in raster order; none: it stays);
    regions are numbered 0..n_b-1 per image in raster order of their first pixel, the batch-wide node index is offsets[b] + label.
    10 + 9 rounds launches whatever the contents, no host synchronisation."""
    if not isinstance(raw, torch.Tensor) or raw.dtype != torch.int32 or raw.dim() != 3:
        raise TypeError("connect_regions: raw must be an int32 (B, H, W) tensor")
    _lib.require_hip(raw, "connect_regions")
    min_area, rounds = int(min_area), int(rounds)
    if min_area < 0 or not 0 <= rounds <= MAX_ROUNDS:
        raise ValueError(f"min_area must be >= 0 and rounds in 0..{MAX_ROUNDS}, got {min_area}, {rounds}")
    raw = raw.contiguous()
    B, H, W = raw.shape
    labels = torch.empty_like(raw)
    counts = torch.zeros(B, device=raw.device, dtype=torch.int64)
    offsets = torch.zeros(B + 1, device=raw.device, dtype=torch.int64)
    _lib.call("mgu_regions_connect", raw.device, raw, B, H, W, min_area, rounds, labels, counts, offsets)
    return labels, counts, offsets


def region_adjacency(labels: torch.Tensor, offsets: torch.Tensor, node_capacity: int, edge_capacity: int = None):
    """The region adjacency graph of an int32 label map (B, H, W) with offsets (labels < 0 or >= n_b take no part) ->
    (rowptr int32 (node_capacity + 1), col int32 (edge_capacity), border int32 (edge_capacity), status int32 (1)): both directions
    of every edge, rows by batch-wide node index, columns ascending, no self loops; border = the number of pixel edges between the
    two regions.  edge_capacity defaults to 6 node_capacity (a planar graph has at most 6 N - 12 directed edges).  status: 1 = more
    edges than edge_capacity (rowptr still holds the true prefix sums), 2 = an image's nodes pass node_capacity (it contributes
    nothing).  6 launches, no host synchronisation."""
    labels, offsets = _labels(labels, offsets, "region_adjacency")
    ncap = int(node_capacity)
    ecap = 6 * ncap if edge_capacity is None else int(edge_capacity)
    if ncap < 0 or ecap < 0:
        raise ValueError("capacities must be >= 0")
    B, H, W = labels.shape
    dev = labels.device
    rowptr = torch.zeros(ncap + 1, device=dev, dtype=torch.int32)
    col = torch.zeros(ecap, device=dev, dtype=torch.int32)
    border = torch.zeros(ecap, device=dev, dtype=torch.int32)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("mgu_regions_adjacency", dev, labels, offsets, B, H, W, ncap, ecap, rowptr, col if ecap else None, border if ecap else None,
              status)
    return rowptr, col, border, status


def region_features(images_u8, labels: torch.Tensor, offsets: torch.Tensor, node_capacity: int, return_stats: bool = False):
    """Node features float32 (node_capacity, 8) of the regions of `labels` in the photographs: [mean L / 100, mean a / 128, mean b /
    128, (mean x + 1/2) / W, (mean y + 1/2) / H, area / (H W), 0, 0] from exact integer sums (include/mgunet.h has the expressions);
    rows of no node are zero.  return_stats: also int64 (node_capacity, 6) [area, sum x, sum y, sum L, sum a, sum b]."""
    labels, offsets = _labels(labels, offsets, "region_features")
    img = _images(images_u8, "region_features")
    B, H, W = labels.shape
    if tuple(img.shape[:3]) != (B, H, W) or img.device != labels.device:
        raise ValueError(f"region_features: images {tuple(img.shape)} do not match labels {(B, H, W)} (or live on another device)")
    ncap = int(node_capacity)
    if ncap < 0:
        raise ValueError("node_capacity must be >= 0")
    feat = torch.zeros((ncap, FEATURE_WIDTH), device=img.device, dtype=torch.float32)
    stats = torch.zeros((ncap, 6), device=img.device, dtype=torch.int64) if return_stats else None
    _lib.call("mgu_regions_features_u8", img.device, img, labels, offsets, B, H, W, *_table_args(), ncap, feat, stats)
    return (feat, stats) if return_stats else feat


def _nhwc_view(feat: torch.Tensor):
    """(tensor holding the storage, pitch) of the (B, C, H, W) view `feat` when its channels are unit-stride inside NHWC rows of
    some pitch >= C (a UNet.forward output, or a channel slice of one): read in place; anything else costs one copy."""
    B, Cc, H, W = feat.shape
    sn, sc, sh, sw = feat.stride()
    if sc == 1 and sw >= Cc and sh == W * sw and sn == H * sh:
        return feat, sw
    return nhwc_storage(feat), Cc


def region_pool(feat: torch.Tensor, labels: torch.Tensor, offsets: torch.Tensor, node_capacity: int) -> torch.Tensor:
    """Means of a float32 feature map over the regions: feat (B, D, H, W) at the label map's resolution -- the NCHW view of NHWC
    storage every UNet.forward output is, or a channel slice of one (both read in place) -> float32 (node_capacity, D).  Each value
    is quantised to round_half_even(clamp(v, -65536, 65536) 2^20) (NaN counts as 0) and summed in int64 with integer atomics: exact,
    order-free, bitwise reproducible, within 2^-21 + 2^-24 |mean| of the float64 mean.  Rows of no node are zero.  No backward."""
    labels, offsets = _labels(labels, offsets, "region_pool")
    if not isinstance(feat, torch.Tensor) or feat.dtype != torch.float32 or feat.dim() != 4:
        raise TypeError("region_pool: feat must be a (B, D, H, W) float32 tensor")
    _lib.require_hip(feat, "region_pool")
    B, H, W = labels.shape
    if (feat.shape[0], feat.shape[2], feat.shape[3]) != (B, H, W) or feat.device != labels.device or feat.shape[1] < 1:
        raise ValueError(f"region_pool: feat {tuple(feat.shape)} does not match labels {(B, H, W)} (or lives on another device)")
    ncap = int(node_capacity)
    if ncap < 0:
        raise ValueError("node_capacity must be >= 0")
    D = feat.shape[1]
    x, ld = _nhwc_view(feat)
    out = torch.zeros((ncap, D), device=feat.device, dtype=torch.float32)
    _lib.call("mgu_regions_pool_nhwc", feat.device, x, int(ld), 0, D, labels, offsets, B, H, W, ncap, out)
    return out


@dataclass
class SuperpixelGraph:
    """What superpixel_graph returns, all on the device.  labels int32 (B, H, W): the region of every pixel, 0..n_b-1 per image;
    counts int64 (B), offsets int64 (B + 1): node offsets[b] + label is the batch-wide row of a region; rowptr int32 (node_capacity +
    1), col, border int32 (edge_capacity): the adjacency CSR (columns ascending, both directions, border = shared pixel edges);
    features float32 (node_capacity, 8); graph_ptr int32 (B + 1) = offsets, the GAT's per-graph node ranges; status int32 (1), see
    region_adjacency.  rowptr, col and graph_ptr go to gat_forward_csr as they are, labels to FeatureFusion(region_to_pixel_map=)
    after adding offsets[b] per image (node_map())."""
    labels: torch.Tensor
    counts: torch.Tensor
    offsets: torch.Tensor
    rowptr: torch.Tensor
    col: torch.Tensor
    border: torch.Tensor
    features: torch.Tensor
    graph_ptr: torch.Tensor
    status: torch.Tensor

    @property
    def node_capacity(self) -> int:
        return self.rowptr.numel() - 1

    @property
    def edge_capacity(self) -> int:
        return self.col.numel()

    def check(self) -> "SuperpixelGraph":
        """Raise unless the graph is complete (synchronises)."""
        st = int(self.status.item())
        if st:
            why = [w for bit, w in ((1, f"more directed edges than edge_capacity = {self.edge_capacity}"),
                                    (2, f"an image's nodes pass node_capacity = {self.node_capacity}")) if st & bit]
            raise RuntimeError("superpixel graph incomplete: " + "; ".join(why))
        return self

    def edge_index(self) -> torch.Tensor:
        """The edges as COO int64 (2, E), [source; target] in CSR order, for GATNetwork.forward (synchronises to learn E)."""
        E = min(int(self.rowptr[-1].item()), self.edge_capacity)
        deg = (self.rowptr[1:] - self.rowptr[:-1]).to(torch.int64)
        tgt = torch.repeat_interleave(torch.arange(self.node_capacity, device=self.rowptr.device), deg)[:E]
        return torch.stack([self.col[:E].to(torch.int64), tgt])

    def node_map(self) -> torch.Tensor:
        """int64 (B, H, W): the batch-wide node index offsets[b] + label of every pixel."""
        return self.labels.to(torch.int64) + self.offsets[:-1].view(-1, 1, 1)

    def pool(self, feat: torch.Tensor) -> torch.Tensor:
        """region_pool of feat (B, D, H, W) over this graph's regions: float32 (node_capacity, D)."""
        return region_pool(feat, self.labels, self.offsets, self.node_capacity)


def superpixel_graph(images_u8, step: int = None, n_segments: int = None, compactness: float = 10.0, iterations: int = 10,
                     min_area: int = None, rounds: int = 2, node_capacity: int = None, edge_capacity: int = None,
                     smoother=None) -> SuperpixelGraph:
    """slic_labels -> connect_regions -> region_adjacency + region_features on a uint8 batch, nothing read back in between.
    min_area defaults to step^2 / 4, rounds to 2 (one round leaves the small regions whose only neighbours were small).
    node_capacity defaults to 4 B gx gy and edge_capacity to 6 node_capacity (regions are connected, so the graph is planar); the
    status word is checked lazily by SuperpixelGraph.check().  smoother: a GaussianSmoother whose blur the SLIC stage segments instead
    of the photograph (noise fragments the raw labels); the node features are still taken from the photograph itself."""
    img = _images(images_u8, "superpixel_graph") if isinstance(images_u8, (np.ndarray, torch.Tensor)) else None
    if img is None:
        raise TypeError("superpixel_graph: images must be a uint8 numpy array or tensor")
    B, H, W = img.shape[:3]
    S = _step(H, W, step, n_segments)
    seg = smoother.smooth(img) if smoother is not None else img
    raw = slic_labels(seg, step=S, compactness=compactness, iterations=iterations)
    labels, counts, offsets = connect_regions(raw, (S * S) // 4 if min_area is None else min_area, rounds)
    gx, gy = -(-W // S), -(-H // S)
    ncap = 4 * B * gx * gy if node_capacity is None else int(node_capacity)
    rowptr, col, border, status = region_adjacency(labels, offsets, ncap, edge_capacity)
    features = region_features(img, labels, offsets, ncap)
    return SuperpixelGraph(labels, counts, offsets, rowptr, col, border, features, offsets.to(torch.int32), status)
