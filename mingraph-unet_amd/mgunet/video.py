"""Counting over a video: frame registration and object tracks (csrc/video.hip; include/mgunet.h, "video").

The reference records video while walking along a row and cuts it into frames (data_collection/video_capture.py,
frame_extractor.py); consecutive frames overlap by most of their area, so the sum of per-frame counts counts every fruit several
times.  This module says how far the scene moved between two frames (frame_shifts: an exhaustive byte-SAD search, coarse to fine),
which objects of the next frame continue objects of the previous one (link_objects: both label maps in one coordinate frame, cut to
the common rectangle, then the overlap table and the greedy matcher of the instance evaluation on the VISIBLE areas) and which track
every object belongs to (track_ids).  VideoCounter strings them together over chunks of a long video.  This build's own definition:
integers only, bitwise repeatable, a fixed number of launches, nothing is read back to the host before compute().

Out of scope: the motion model is one global integer translation per frame pair (no rotation, zoom or per-object parallax); links go
only between consecutive frames (no re-identification after a missed frame, no motion model)."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .engine import argmax_classes
from .instances import _overlaps, _sides
from .objects import ObjectTable, _clean, _label, _ObjectEvaluator, _split, _stats

FACTORS = (1, 2, 4, 8)
MAX_RADIUS = 32


def _frames(frames: torch.Tensor, what: str):
    _lib.require_hip(frames, what)
    if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] != 3):
        raise TypeError(f"{what}: frames must be uint8 (T, H, W, 3) or (T, H, W), got {frames.dtype} {tuple(frames.shape)}")
    return frames.contiguous(), 3 if frames.dim() == 4 else 1


def frame_shifts(frames: torch.Tensor, radius: int = 16, factor: int = 2, bgr: bool = False, return_surface: bool = False):
    """How far the scene moved between consecutive frames: int32 (T-1, 2) [dy, dx] in pixels -- a scene point at p in frame t lies at
    p + shift in frame t+1 -- and int64 (T-1, 2) [the cost at that shift, the cost at the last level's zero offset], on the device.

    frames: uint8 (T, H, W, 3) (RGB, or BGR with bgr=True) or grey (T, H, W), T >= 2.  The luma byte (77 R + 150 G + 29 B + 128) >> 8
    is averaged over factor x factor blocks (factor 1, 2, 4 or 8; trailing rows and columns dropped); on that coarse plane every shift
    s in [-radius, radius]^2 (radius 1..32, in coarse pixels) costs the sum of |A(p) - B(p + s)| over the window that keeps `radius`
    pixels from every edge -- the same window for every shift, at least 8 x 8.  The smallest cost wins; ties go to the smallest
    sy^2 + sx^2, then the smaller sy, then the smaller sx (two uniform frames: (0, 0)).  With factor > 1 the choice is refined on the
    full-resolution luma among factor * s + d, d in [-factor, factor]^2, the same way, without a host round trip.  return_surface:
    also the int64 (T-1, 2 radius + 1, 2 radius + 1) coarse cost surface, whose minimum's sharpness tells how far to trust the shift.
    One global integer translation per pair: no rotation, zoom or parallax."""
    frames, ch = _frames(frames, "frame_shifts")
    T, H, W = frames.shape[:3]
    R, f = int(radius), int(factor)
    if T < 2:
        raise ValueError(f"frame_shifts: at least 2 frames, got {T}")
    dev = frames.device
    shifts = torch.empty((T - 1, 2), device=dev, dtype=torch.int32)
    cost = torch.empty((T - 1, 2), device=dev, dtype=torch.int64)
    surface = torch.empty((T - 1, 2 * R + 1, 2 * R + 1), device=dev, dtype=torch.int64) if return_surface and 1 <= R <= MAX_RADIUS else None
    _lib.call("mgu_frame_shifts", dev, frames, T, H, W, ch, int(bool(bgr)), R, f, shifts, cost, surface)
    return (shifts, cost, surface) if return_surface else (shifts, cost)


def _link(labels, offsets, cls, cap, shifts, T, H, W, iou_dev, scores, bufs, status):
    """Align the T frames' label maps pair by pair, build the overlap table of the pairs and match on the visible areas into
    bufs["match"][0] (1, cap): row 0 is the link table.  The next-frame side's offsets are offsets[1:]: they do not start at 0, which
    mgu_object_overlaps and mgu_match_masks take as it is (their indices are batch-wide)."""
    prev, nxt, vp, vn = bufs["aligned"]
    dev = labels.device
    _lib.call("mgu_track_align", dev, labels, offsets, int(cap), shifts, T, H, W, prev, nxt, vp, vn)
    _overlaps(prev, offsets, cap, nxt, offsets[1:], cap, T - 1, H, W, *bufs["pairs"], status)
    mg, mi = bufs["match"]
    mg.fill_(-1)
    _lib.call("mgu_match_masks", dev, T - 1, *_sides(bufs["pairs"], offsets, cls, vp, cap, offsets[1:], cls, vn, cap), scores, iou_dev, 1, mg, mi,
              bufs["totals"])
    return mg[0]


def _link_buffers(dev, cap, npix_pairs):
    mk = lambda shape, dt: torch.empty(shape, device=dev, dtype=dt)  # noqa: E731
    return {"aligned": (mk(npix_pairs, torch.int32), mk(npix_pairs, torch.int32), mk(max(cap, 1), torch.int64), mk(max(cap, 1), torch.int64)),
            "pairs": (mk(cap + 1, torch.int64), mk(npix_pairs, torch.int64), mk(npix_pairs, torch.int64)),
            "match": (mk((1, max(cap, 1)), torch.int64), mk((1, max(cap, 1)), torch.float64)),
            "totals": torch.zeros((1, 3), device=dev, dtype=torch.int64)}


def _iou(iou: float) -> float:
    if not 0.0 < iou <= 1.0:
        raise ValueError(f"iou must lie in (0, 1], got {iou}")
    return float(iou)


def link_objects(table: ObjectTable, shifts: torch.Tensor, iou: float = 0.3, scores: torch.Tensor = None, return_aligned: bool = False):
    """For every object of the T frames of `table` (connected_components / split_objects of the frames as one batch) the batch-wide
    index of its predecessor in the frame before, or -1: int64 (N) on the device; the objects of frame 0 have none.

    shifts: int32 (T-1, 2) on the device (frame_shifts).  Per pair the previous frame's labels are moved by the shift and both maps are
    cut to the common rectangle of the two frames, so a fruit half inside frame t and whole in frame t+1 is compared on the part both
    frames see.  The objects of the next frame are visited in list order, or by descending `scores` (float32 per object); each takes
    the unused object of the previous frame of its class with the largest IoU = inter / (visible_prev + visible_next - inter) (ties:
    the smaller index) if that IoU is >= iou (mgunet.match_masks' rule).  return_aligned: also (prev_aligned, next_cropped, vis_prev,
    vis_next), the int32 (T-1, H, W) maps and the int64 (N) visible areas.  A fixed number of launches, no host synchronisation."""
    _lib.require_hip(table.labels, "link_objects")
    T, H, W = table.labels.shape
    dev = table.labels.device
    N = table.class_id.numel()
    thr = torch.tensor([_iou(iou)], dtype=torch.float64).to(dev)
    if T < 2:
        raise ValueError("link_objects: at least 2 frames")
    if shifts.dtype != torch.int32 or tuple(shifts.shape) != (T - 1, 2) or shifts.device != dev:
        raise ValueError(f"shifts must be int32 ({T - 1}, 2) on {dev}")
    if scores is not None and (scores.dtype != torch.float32 or scores.numel() != N or scores.device != dev):
        raise ValueError(f"scores must be float32, one per object ({N}), on {dev}")
    bufs = _link_buffers(dev, N, (T - 1) * H * W)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    link = _link(table.labels, table.offsets, table.class_id, N, shifts.contiguous(), T, H, W, thr, None if scores is None else scores.contiguous(),
                 bufs, status)[:N]
    if return_aligned:
        prev, nxt, vp, vn = bufs["aligned"]
        return link, (prev.view(T - 1, H, W), nxt.view(T - 1, H, W), vp[:N], vn[:N])
    return link


def _ids(offsets, T, cap, link, cls, first_ids, next_id, track_id, track_len, track_cls, status):
    _lib.call("mgu_track_ids", offsets.device, offsets, T, int(cap), link, cls, first_ids, next_id, track_id, track_len, track_cls, track_len.numel(),
              status)


def track_ids(offsets: torch.Tensor, link: torch.Tensor, class_id: torch.Tensor, first_ids: torch.Tensor = None, next_id: torch.Tensor = None,
              track_capacity: int = None, tracks=None):
    """Track ids from a link table: (track_id int64 (N), next_id int64 (1), track_len int32 (track_capacity), track_class int64
    (track_capacity), status int32 (1)), all on the device.

    offsets int64 (T+1), link int64 (N) (link_objects) and class_id int64 (N) of the frames' objects.  One workgroup walks the frames
    in order: an object takes its predecessor's id, an unlinked one the next fresh id in object order.  To continue a video across
    calls pass the next call the previous call's last frame as its frame 0 with first_ids = that frame's ids (they are kept and the
    frame is not counted twice), next_id = the returned scalar (updated in place) and tracks = (track_len, track_class) (accumulated
    in place).  track_len[k]: frames in which track k has an object; track_class[k]: the class of its first object.  status bit 1: an
    id reached track_capacity (default: N for a fresh start); nothing is written past the arrays."""
    _lib.require_hip(offsets, "track_ids")
    dev = offsets.device
    T, N = offsets.numel() - 1, class_id.numel()
    if link.numel() != N or link.dtype != torch.int64 or class_id.dtype != torch.int64 or offsets.dtype != torch.int64:
        raise ValueError("track_ids: offsets, link and class_id must be int64, link and class_id of one length")
    if next_id is None:
        next_id = torch.zeros(1, device=dev, dtype=torch.int64)
    if tracks is None:
        cap = N if track_capacity is None else int(track_capacity)
        tracks = (torch.zeros(max(cap, 0), device=dev, dtype=torch.int32), torch.full((max(cap, 0),), -1, device=dev, dtype=torch.int64))
    track_len, track_cls = tracks
    if first_ids is not None and first_ids.dtype != torch.int64:
        raise ValueError("track_ids: first_ids must be int64")
    track_id = torch.full((N,), -1, device=dev, dtype=torch.int64)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _ids(offsets, T, N, link.contiguous(), class_id.contiguous(), first_ids, next_id, track_id, track_len, track_cls, status)
    return track_id, next_id, track_len, track_cls, status


class VideoCounter(_ObjectEvaluator):
    """Count the objects of a video once each.  update(frames_u8, logits_or_labels) takes a chunk of consecutive frames -- uint8
    (B, H, W, 3) or (B, H, W) -- with the network's (B, C, H, W) float32 logits or an integer (B, H, W) class map: the class map is
    cleaned (`clean`: a dict of clean_masks' parameters), labelled (connectivity, min_area), split (`split`: a dict of split_objects'
    parameters), the frames are registered (radius, factor, bgr: frame_shifts), the objects linked (iou: link_objects) and numbered
    (track_ids).  The last frame, its class map and its ids are carried into the next chunk, so chunks of any sizes give the ids of
    one call over the whole video.  Every buffer is sized for the worst case and nothing is read back: update() never blocks the host.
    compute() synchronises once and returns a dictionary: 'tracks' (tracks started), 'tracks_per_class', 'count' (tracks seen in at
    least min_length frames: the count of the video) and 'count_per_class', 'frame_count_sum' (the plain sum of the per-frame counts,
    for comparison), 'frames', 'track_lengths' and 'track_classes' (numpy, one entry per track), 'shifts' (numpy int32 (frames-1, 2))
    and 'track_ids' (a list with one int64 numpy array per frame, in object order).  max_tracks: the capacity of the per-track arrays;
    compute() raises when the video starts more tracks."""

    CLASS_RANGE = (2, None)

    def __init__(self, num_classes: int, device, radius: int = 16, factor: int = 2, iou: float = 0.3, min_length: int = 2, connectivity: int = 2,
                 min_area: int = 0, clean: dict = None, split: dict = None, bgr: bool = False, max_tracks: int = 65536):
        super().__init__(num_classes, device, connectivity, min_area, split, clean)
        if not 1 <= int(radius) <= MAX_RADIUS or int(factor) not in FACTORS:
            raise ValueError(f"radius must be in 1..{MAX_RADIUS} and factor one of {FACTORS}")
        if min_length < 1 or max_tracks < 1:
            raise ValueError("min_length and max_tracks must be >= 1")
        self.radius, self.factor, self.iou, self.min_length, self.bgr = int(radius), int(factor), _iou(iou), int(min_length), bool(bgr)
        self.max_tracks = int(max_tracks)
        self._thr = torch.tensor([self.iou], dtype=torch.float64).to(self.device)
        self._shape = None
        self.reset()

    def reset(self) -> None:
        dev = self.device
        self.next_id = torch.zeros(1, device=dev, dtype=torch.int64)
        self.track_len = torch.zeros(self.max_tracks, device=dev, dtype=torch.int32)
        self.track_class = torch.full((self.max_tracks,), -1, device=dev, dtype=torch.int64)
        self.status = torch.zeros(1, device=dev, dtype=torch.int32)      # mgu_track_ids' bits
        self.pair_status = torch.zeros(1, device=dev, dtype=torch.int32)  # mgu_object_overlaps' bits
        self._carry = None        # (frame, class map, ids of its objects (H*W))
        self._counts, self._shifts, self._ids_rec = [], [], []

    def _buffers(self, T, H, W):
        n = T * H * W
        if (n, H, W) != self._shape:
            mk = lambda shape, dt: torch.empty(shape, device=self.device, dtype=dt)  # noqa: E731
            b = _link_buffers(self.device, n, max(T - 1, 1) * H * W)
            b["objects"] = (mk(n, torch.int32), mk(n, torch.int64), mk((n, 4), torch.int32), mk(n, torch.int64))
            b["ids"] = mk(n, torch.int64)
            b["nolink"] = torch.full((n,), -1, device=self.device, dtype=torch.int64)
            b["arange"] = torch.arange(H * W, device=self.device)
            self._bufs, self._shape = b, (n, H, W)
        return self._bufs

    def _class_map(self, x, B, H, W):
        if x.is_floating_point():
            if x.dim() != 4 or x.dtype != torch.float32 or tuple(x.shape) != (B, x.shape[1], H, W):
                raise ValueError(f"logits must be float32 ({B}, C, {H}, {W}), got {tuple(x.shape)}")
            if self._clean is None:
                return argmax_classes(x)
            from ._args import nhwc_storage
            out = torch.empty((B, H, W), device=self.device, dtype=torch.int64)
            _clean(nhwc_storage(x), 1, B, H, W, x.shape[1], x.shape[1], self._clean, out, None)
            return out
        if tuple(x.shape) != (B, H, W):
            raise ValueError(f"a class map must be ({B}, {H}, {W}), got {tuple(x.shape)}")
        m = x.to(self.device, torch.int64).contiguous()
        if self._clean is None:
            return m
        out = torch.empty_like(m)
        _clean(m, 0, B, H, W, 0, self.num_classes, self._clean, out, None)
        return out

    def update(self, frames_u8: torch.Tensor, logits_or_labels: torch.Tensor) -> None:
        """Add the next chunk of consecutive frames (any number >= 1) with its logits or class map."""
        frames, _ = _frames(frames_u8.to(self.device), "VideoCounter")
        B, H, W = frames.shape[:3]
        cm = self._class_map(logits_or_labels, B, H, W)
        carried = self._carry is not None
        if carried:
            if self._carry[0].shape != frames.shape[1:]:
                raise ValueError("VideoCounter: the frames of a video must keep one shape")
            frames, cm = torch.cat([self._carry[0][None], frames]), torch.cat([self._carry[1][None], cm])
        T = frames.shape[0]
        bufs = self._buffers(T, H, W)
        cap = self._shape[0]
        lab, cls, bbox, area = bufs["objects"]
        lab = lab.view(T, H, W)
        counts = torch.empty(T, device=self.device, dtype=torch.int64)
        offsets = torch.empty(T + 1, device=self.device, dtype=torch.int64)
        _label(cm, 0, T, H, W, 0, self.connectivity, 0, self.num_classes, self.min_area, lab, counts, offsets)
        if self._split is not None:
            _split(lab, T, H, W, self._split, lab, counts, offsets)
        _stats(lab, cm, 0, T, H, W, 0, offsets, cap, cls, bbox, area)
        link = bufs["nolink"]
        if T >= 2:
            shifts, _ = frame_shifts(frames, self.radius, self.factor, self.bgr)
            link = _link(lab, offsets, cls, cap, shifts, T, H, W, self._thr, None, bufs, self.pair_status)
            self._shifts.append(shifts)
        ids = bufs["ids"]
        _ids(offsets, T, cap, link, cls, self._carry[2] if carried else None, self.next_id, ids, self.track_len, self.track_class, self.status)
        rows = (offsets[T - 1] + bufs["arange"]).clamp_(max=cap - 1)      # the last frame's rows (those past its objects are not read)
        self._carry = (frames[-1].clone(), cm[-1].clone(), ids[rows])
        first = 1 if carried else 0
        self._counts.append(counts[first:])
        self._ids_rec.append((ids.clone(), offsets[first:].clone()))

    def compute(self) -> dict:
        """Synchronise once and return the dictionary described above over every chunk since the last reset()."""
        st, pst = int(self.status.item()), int(self.pair_status.item())
        if st or pst:
            raise RuntimeError(f"VideoCounter: track status {st} (1: more than max_tracks = {self.max_tracks} tracks, 2: object capacity), "
                               f"overlap status {pst}")
        n = int(self.next_id.item())
        lengths, classes = self.track_len[:n].cpu().numpy(), self.track_class[:n].cpu().numpy()
        counted = lengths >= self.min_length
        per_class = lambda sel: np.bincount(classes[sel], minlength=self.num_classes)[:self.num_classes].tolist()  # noqa: E731
        counts = torch.cat(self._counts).cpu().numpy() if self._counts else np.zeros(0, np.int64)
        shifts = torch.cat(self._shifts).cpu().numpy() if self._shifts else np.zeros((0, 2), np.int32)
        per_frame = []
        for ids, off in self._ids_rec:
            ids, off = ids.cpu().numpy(), off.cpu().numpy()
            per_frame += [ids[off[k]:off[k + 1]] for k in range(len(off) - 1)]
        return {"tracks": n, "tracks_per_class": per_class(np.ones(n, bool)), "count": int(counted.sum()), "count_per_class": per_class(counted),
                "frame_count_sum": int(counts.sum()), "frames": int(counts.size), "track_lengths": lengths, "track_classes": classes,
                "shifts": shifts, "track_ids": per_frame}


def count_video(model, frames: torch.Tensor, chunk: int = 8, num_classes: int = None, preprocess=None, **counter) -> dict:
    """Count the objects of a video: for every chunk of `chunk` frames logits = model(preprocess(frames)) under torch.no_grad() in eval
    mode, then VideoCounter.update.  frames: uint8 (T, H, W, 3) (moved to the model's device chunk by chunk).  preprocess: uint8
    (B, H, W, 3) on the device -> the model's (B, 3, H, W) float32 input; default: ToTensor's x / 255.  `counter`: VideoCounter's
    keywords (radius, factor, iou, min_length, connectivity, min_area, clean, split, bgr, max_tracks).  Returns VideoCounter.compute()'s
    dictionary; the model's training flag is restored."""
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    dev = next(model.parameters()).device
    vc = VideoCounter(int(num_classes if num_classes is not None else model.num_classes), dev, **counter)
    if preprocess is None:
        preprocess = lambda u8: (u8.to(torch.float32) / 255.0).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for i in range(0, frames.shape[0], chunk):
                u8 = frames[i:i + chunk].to(dev)
                out = model(preprocess(u8))
                vc.update(u8, out[0] if isinstance(out, (tuple, list)) else out)
        return vc.compute()
    finally:
        model.train(was_training)
