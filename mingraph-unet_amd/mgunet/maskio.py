"""Masks in and out of the device (csrc/maskio.hip): the int32 label map every object stage works on against the two forms that
annotation tools and result files use -- COCO's run-length encoding and polygons.

Out: encode_masks gives the runs of every object in COCO's column-major order (RunTable.to_coco: one RLE per instance),
object_outlines the closed polygons of every object on the pixel grid (OutlineTable.to_polygons / to_coco).  In: runs_from_coco +
labels_from_runs and rasterize_polygons give the label map of COCO annotations, objects_from_annotations the ObjectTable that
object_overlaps, match_masks, panoptic_totals and border_weights take.  The reference has no such stage (it reads class PNGs): the
definitions are this build's own, in integers, bitwise equal to tests/maskio_oracle.py.  The device calls
never synchronise; the `check()` of a table does, and so does whatever hands Python lists back."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .objects import ObjectTable, _table


# ---- COCO's compressed counts, after the published maskApi.c (rleToString / rleFrString) ------------------------------------------------
def rle_to_string(counts) -> str:
    """COCO's compressed form of the counts of one RLE: counts from the fourth on are stored as differences from the count two
    before; every value goes out 5 bits at a time, least significant first, with bit 0x20 set while more follow (a group's bit 0x10
    is the sign the decoder extends), each group as the character chr(48 + group).  Written after maskApi.c; not compared with a
    pycocotools build (none is installed here), only by round trip and on a vector worked by hand."""
    out = []
    counts = [int(c) for c in counts]
    for i, x in enumerate(counts):
        if i > 2:
            x -= counts[i - 2]
        more = True
        while more:
            c = x & 0x1F
            x >>= 5                                  # arithmetic: -1 stays -1
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def rle_from_string(s: str) -> list:
    """The counts of a compressed COCO RLE string (the inverse of rle_to_string)."""
    counts, p = [], 0
    data = s.encode("ascii") if isinstance(s, str) else bytes(s)
    while p < len(data):
        x, k, more = 0, 0, True
        while more:
            if p >= len(data):
                raise ValueError("rle_from_string: the string ends inside a count")
            c = data[p] - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p, k = p + 1, k + 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def _status(status: torch.Tensor, what: str, bits) -> None:
    st = int(status.item())
    if st:
        raise RuntimeError(f"{what} incomplete: " + "; ".join(w for bit, w in bits if st & bit))


def _labelled(x, what: str):
    """(labels int32 (B, H, W), offsets int64 (B + 1), N) of an ObjectTable or a (labels, offsets) pair; the pair costs one
    synchronisation to read N = offsets[B]."""
    if isinstance(x, ObjectTable):
        labels, offsets, N = x.labels, x.offsets, x.class_id.numel()
    else:
        labels, offsets = x
        N = None
    _lib.require_hip(labels, what)
    if labels.dim() != 3 or labels.dtype != torch.int32 or offsets.dtype != torch.int64 or offsets.numel() != labels.shape[0] + 1:
        raise TypeError(f"{what}: labels must be int32 (B, H, W) and offsets int64 (B + 1)")
    if N is None:
        N = int(offsets[-1].item())
    return labels.contiguous(), offsets.contiguous(), N


def _capacity(given, default: int, name: str) -> int:
    cap = default if given is None else int(given)
    if cap < 0:
        raise ValueError(f"{name} must be >= 0")
    return cap


# ---- runs ----------------------------------------------------------------------------------------------------------------------------
@dataclass
class RunTable:
    """The runs of the objects of a batch in COCO's order, CSR by object, all on the device.  The position of pixel (x, y) is
    p = x * H + y.  run_ptr: int64 (N + 1), the runs of batch-wide object i are [run_ptr[i], run_ptr[i + 1]).  run_start, run_length:
    int32 (run_capacity), ascending inside an object.  status: int32 (1): bit 1 = more runs than run_capacity (the surplus is
    dropped), bit 2 = objects past the per-object arrays.  offsets: int64 (B + 1), the objects of image b are rows
    [offsets[b], offsets[b + 1]).  size: (B, H, W)."""
    run_ptr: torch.Tensor
    run_start: torch.Tensor
    run_length: torch.Tensor
    status: torch.Tensor
    offsets: torch.Tensor
    size: tuple

    @property
    def run_capacity(self) -> int:
        return self.run_start.numel()

    def check(self) -> "RunTable":
        """Raise unless the table is complete (synchronises)."""
        _status(self.status, "run table", ((1, f"more runs than run_capacity = {self.run_capacity}"),
                                           (2, "objects pass the per-object arrays")))
        return self

    def areas(self) -> torch.Tensor:
        """int64 (N): the pixels of every object, the sum of its run lengths (device; no synchronisation).  Equals ObjectTable.area
        for a table that is complete."""
        cap = self.run_capacity
        csum = torch.cat([torch.zeros(1, device=self.run_ptr.device, dtype=torch.int64), torch.cumsum(self.run_length.to(torch.int64), 0)])
        ptr = self.run_ptr.clamp(max=cap)
        return csum[ptr[1:]] - csum[ptr[:-1]]

    def to_coco(self, compress: bool = True) -> list:
        """Per image, one COCO RLE per object in label order: {"size": [H, W], "counts": ...}.  counts = [start0, len0, gap, len1,
        ...] -- zeros first, then alternating -- with a trailing zero-run when the mask does not end the image, formed on the host
        from the run arrays (synchronises); as COCO's compressed string (rle_to_string), or as the list with compress=False."""
        self.check()
        B, H, W = self.size
        ptr, off = self.run_ptr.cpu().numpy(), self.offsets.cpu().numpy()
        start, length = self.run_start.cpu().numpy().astype(np.int64), self.run_length.cpu().numpy().astype(np.int64)
        out = []
        for b in range(B):
            rles = []
            for i in range(int(off[b]), int(off[b + 1])):
                s, n = start[ptr[i]:ptr[i + 1]], length[ptr[i]:ptr[i + 1]]
                counts = np.empty(2 * s.size, np.int64)
                counts[0::2] = s - np.concatenate(([0], (s + n)[:-1]))
                counts[1::2] = n
                end = int((s + n)[-1]) if s.size else 0
                counts = counts.tolist() + ([H * W - end] if end < H * W else [])
                rles.append({"size": [H, W], "counts": rle_to_string(counts) if compress else counts})
            out.append(rles)
        return out


def encode_masks(objects, run_capacity: int = None) -> RunTable:
    """The run table of an ObjectTable (connected_components / split_objects) or of a (labels int32 (B, H, W), offsets int64 (B + 1))
    pair; a pixel whose label lies outside [1, n_b] belongs to no object.  run_capacity: the length of the run arrays; the default
    B*H*W can never overflow (a run holds at least one pixel and no pixel lies in two runs, so runs <= pixels).  A fixed number of
    launches, no host synchronisation (`check()` synchronises)."""
    labels, offsets, N = _labelled(objects, "encode_masks")
    B, H, W = labels.shape
    dev = labels.device
    cap = _capacity(run_capacity, B * H * W, "run_capacity")
    run_ptr = torch.empty(N + 1, device=dev, dtype=torch.int64)
    run_start = torch.zeros(cap, device=dev, dtype=torch.int32)
    run_length = torch.zeros(cap, device=dev, dtype=torch.int32)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("mgu_mask_runs", dev, labels, offsets, N, B, H, W, cap, run_ptr, run_start, run_length, status)
    return RunTable(run_ptr, run_start, run_length, status, offsets, (B, H, W))


def _rle_counts(rle) -> list:
    counts = rle["counts"]
    if isinstance(counts, (str, bytes)):
        counts = rle_from_string(counts)
    return [int(c) for c in counts]


def runs_from_coco(rles, device) -> RunTable:
    """The RunTable of COCO annotations: rles is, per image, a list of RLE dicts {"size": [H, W], "counts": string or list}; object
    k of image b is the k-th dict of its list.  Every image must have the same size (an image without objects takes it from the
    others).  Host parsing, one upload."""
    device = torch.device(device)
    _lib.require_hip(device, "runs_from_coco")
    sizes = {tuple(r["size"]) for per in rles for r in per}
    if len(sizes) != 1:
        raise ValueError(f"runs_from_coco: the RLEs must share one size, got {sorted(sizes)}")
    H, W = sizes.pop()
    ptr, start, length, off = [0], [], [], [0]
    for per in rles:
        for r in per:
            counts = _rle_counts(r)
            if sum(counts) != H * W or any(c < 0 for c in counts):
                raise ValueError(f"runs_from_coco: counts do not add up to H * W = {H * W}")
            pos = 0
            for j, c in enumerate(counts):
                if j % 2 == 1 and c > 0:
                    start.append(pos), length.append(c)
                pos += c
            ptr.append(len(start))
        off.append(off[-1] + len(per))
    mk = lambda v, dt: torch.tensor(v, dtype=dt).to(device)  # noqa: E731
    return RunTable(mk(ptr, torch.int64), mk(start, torch.int32), mk(length, torch.int32), torch.zeros(1, device=device, dtype=torch.int32),
                    mk(off, torch.int64), (len(rles), H, W))


def labels_from_runs(runs: RunTable, B: int = None, H: int = None, W: int = None, return_status: bool = False):
    """(labels int32 (B, H, W), counts int64 (B), offsets int64 (B + 1)) of a RunTable: the map is zero, then every run of object k
    of image b paints k over its positions; where objects overlap the LARGEST label wins (COCO annotations do overlap).  B, H, W
    default to runs.size.  A run with start < 0, length < 1 or start + length > H*W paints nothing and sets bit 1 of the status word
    (return_status=True appends it, an int32 (1) device tensor).  One launch and one fill; no host synchronisation."""
    B, H, W = (runs.size[k] if v is None else int(v) for k, v in enumerate((B, H, W)))
    dev = runs.run_ptr.device
    _lib.require_hip(dev, "labels_from_runs")
    if runs.offsets.numel() != B + 1:
        raise ValueError(f"labels_from_runs: offsets of {runs.offsets.numel() - 1} images for B = {B}")
    labels = torch.empty((B, H, W), device=dev, dtype=torch.int32)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("mgu_runs_to_labels", dev, runs.run_ptr, runs.run_start, runs.run_length, runs.run_capacity, runs.offsets,
              runs.run_ptr.numel() - 1, B, H, W, labels, status)
    out = (labels, runs.offsets[1:] - runs.offsets[:-1], runs.offsets)
    return out + (status,) if return_status else out


# ---- outlines ------------------------------------------------------------------------------------------------------------------------
@dataclass
class OutlineTable:
    """The closed polygons of the objects of a batch on the pixel grid, all on the device.  loop_ptr: int64 (N + 1), the loops of
    batch-wide object i are [loop_ptr[i], loop_ptr[i + 1]), by ascending leader (a loop's smallest edge id).  vertex_ptr: int64
    (loop_capacity + 1).  vertices: int32 (vertex_capacity, 2) as (x, y) corner coordinates, 0..W and 0..H, in travel order: clockwise
    on the screen for an outer loop, counter-clockwise for a hole.  loop_area2: int64 (loop_capacity), the shoelace sum: twice the
    enclosed area, > 0 for an outer loop and < 0 for a hole.  status: int32 (1): bit 1 = more loops than loop_capacity, bit 2 = more
    vertices than vertex_capacity (the surplus is dropped), bit 4 = objects past the per-object arrays."""
    loop_ptr: torch.Tensor
    vertex_ptr: torch.Tensor
    vertices: torch.Tensor
    loop_area2: torch.Tensor
    status: torch.Tensor
    offsets: torch.Tensor
    size: tuple
    connectivity: int

    @property
    def loop_capacity(self) -> int:
        return self.loop_area2.numel()

    @property
    def vertex_capacity(self) -> int:
        return self.vertices.shape[0]

    def check(self) -> "OutlineTable":
        """Raise unless the table is complete (synchronises)."""
        _status(self.status, "outline table", ((1, f"more loops than loop_capacity = {self.loop_capacity}"),
                                               (2, f"more vertices than vertex_capacity = {self.vertex_capacity}"),
                                               (4, "objects pass the per-object arrays")))
        return self

    def to_polygons(self, holes: bool = True) -> list:
        """Per image, per object, the list of its loops, each an int32 numpy array (n, 2) of (x, y) corners (host; synchronises).
        holes=False keeps the outer loops only (loop_area2 > 0)."""
        self.check()
        lp, vp, off = self.loop_ptr.cpu().numpy(), self.vertex_ptr.cpu().numpy(), self.offsets.cpu().numpy()
        v, a2 = self.vertices.cpu().numpy(), self.loop_area2.cpu().numpy()
        return [[[v[vp[l]:vp[l + 1]].copy() for l in range(int(lp[i]), int(lp[i + 1])) if holes or a2[l] > 0]
                 for i in range(int(off[b]), int(off[b + 1]))] for b in range(len(off) - 1)]

    def to_coco(self) -> list:
        """Per image, per object, COCO's polygon form: a list of flat [x0, y0, x1, y1, ...] lists, outer loops only.  COCO polygons
        have no holes, so the round trip through them fills the holes of an object."""
        return [[[p.reshape(-1).tolist() for p in loops] for loops in per] for per in self.to_polygons(holes=False)]


def object_outlines(objects, connectivity: int = 2, loop_capacity: int = None, vertex_capacity: int = None) -> OutlineTable:
    """The outlines of an ObjectTable or of a (labels, offsets) pair.  A pixel side belongs to an object's outline when the pixel
    across it is not the object's; the outside of the image counts as "not", so an object cut by the frame is closed along the frame
    (unlike mgunet.boundary's contour, which ignores the frame).  Sides run clockwise around their pixel; where two pixels of an
    object meet only at a corner, connectivity 2 walks across to the diagonal pixel (one loop around both) and connectivity 1 turns
    back along the same pixel (two loops): pass the connectivity the labels were made with.  Loops per object = its pieces + its holes.
    Polygon simplification is not done.

    loop_capacity, vertex_capacity: the lengths of the loop and vertex arrays.  The defaults B*H*W and 4*B*H*W can never overflow: a
    loop has at least 4 vertices, and a vertex is the start of one of the 4 sides of an object pixel, so vertices <= 4 * pixels and
    loops <= pixels; every pixel its own object reaches both.  4*B*H*W < 2^31.  A fixed number of launches for one (H, W) and object
    count; no host synchronisation (`check()` synchronises)."""
    if connectivity not in (1, 2):
        raise ValueError(f"connectivity must be 1 (4-neighbours) or 2 (8-neighbours), got {connectivity}")
    labels, offsets, N = _labelled(objects, "object_outlines")
    B, H, W = labels.shape
    dev = labels.device
    lcap = _capacity(loop_capacity, B * H * W, "loop_capacity")
    vcap = _capacity(vertex_capacity, 4 * B * H * W, "vertex_capacity")
    loop_ptr = torch.empty(N + 1, device=dev, dtype=torch.int64)
    vertex_ptr = torch.empty(lcap + 1, device=dev, dtype=torch.int64)
    vertices = torch.zeros((vcap, 2), device=dev, dtype=torch.int32)
    area2 = torch.zeros(lcap, device=dev, dtype=torch.int64)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("mgu_object_outlines", dev, labels, offsets, N, B, H, W, int(connectivity), lcap, vcap, loop_ptr, vertex_ptr, vertices, area2,
              status)
    return OutlineTable(loop_ptr, vertex_ptr, vertices, area2, status, offsets, (B, H, W), int(connectivity))


# ---- polygon fill --------------------------------------------------------------------------------------------------------------------
def _crossings(vertices: np.ndarray, vertex_ptr: np.ndarray, H: int, frac_bits: int) -> int:
    """The (edge, scanline) pairs mgu_polygons_to_labels keeps for these loops: for every edge the scanlines y in [0, H) with
    ylo <= (2y + 1) * 2^frac_bits < yhi in doubled units."""
    total, S = 0, 1 << frac_bits
    for l in range(len(vertex_ptr) - 1):
        y = 2 * vertices[vertex_ptr[l]:vertex_ptr[l + 1], 1].astype(np.int64)
        if y.size:
            y2 = np.roll(y, -1)
            first = lambda v: np.clip((v + S - 1) >> (frac_bits + 1), 0, H)  # noqa: E731
            total += int((first(np.maximum(y, y2)) - first(np.minimum(y, y2))).sum())
    return total


def rasterize_polygons(polygons, size=None, frac_bits: int = 0, crossing_capacity: int = None, return_status: bool = False, device=None):
    """(labels int32 (B, H, W), counts int64 (B), offsets int64 (B + 1)) of polygons: an OutlineTable (size defaults to its own), or
    per image a list of (class_id, [loops]) with a loop an (n, 2) sequence of (x, y) or COCO's flat [x0, y0, x1, y1, ...] in pixel
    units -- the pixel (x, y) covers [x, x + 1] x [y, y + 1] -- and size = (H, W); object k of image b is the k-th entry of its list (device:
    where the lists go, default the current HIP device).
    Coordinates are rounded to frac_bits (0..4) fraction bits, must stay below 2^24 in that unit, and may lie outside the image.

    Rule: even-odd over all loops of an object, tested at pixel centres, exactly (int64): a hole is a loop inside a loop, a
    self-intersecting loop is filled even-odd and not by winding.  An edge counts for the centre (cx, cy) iff (y0 <= cy) != (y1 <= cy)
    and the edge crosses the centre's scanline left of cx; horizontal edges never count; a centre exactly on an edge is decided by
    those two inequalities alone.  Where objects overlap the largest label wins.  This is NOT COCO's rleFrPoly, which upsamples by 5
    and draws the boundary: results differ along edges.

    crossing_capacity: the (edge, scanline) pairs kept.  The default can never overflow: for an OutlineTable it is 2*B*H*W (an outline
    edge is a run of pixel sides, every vertical side crosses one scanline and a pixel has two), for lists the exact number, counted
    on the host.  return_status appends the int32 (1) status word (bit 1 crossings, 2 table, 4 coordinate range).  A fixed number of
    launches; no host synchronisation."""
    frac_bits = int(frac_bits)
    if not 0 <= frac_bits <= 4:
        raise ValueError("frac_bits must be in 0..4")
    if isinstance(polygons, OutlineTable):
        t = polygons
        if frac_bits:
            raise ValueError("rasterize_polygons: an OutlineTable holds whole pixels (frac_bits = 0)")
        B = t.size[0]
        H, W = t.size[1:] if size is None else (int(v) for v in size)
        cap = _capacity(crossing_capacity, 2 * B * t.size[1] * t.size[2], "crossing_capacity")
        return _fill(t.loop_ptr.device, t.loop_ptr, t.vertex_ptr, t.vertices, t.offsets, B, H, W, 0, cap, return_status)
    if size is None:
        raise ValueError("rasterize_polygons: size = (H, W) is required for polygon lists")
    H, W = (int(v) for v in size)
    lp, vp, vs, off = [0], [0], [], [0]
    for per in polygons:
        for _cls, loops in per:
            for loop in loops:
                a = np.asarray(loop, np.float64).reshape(-1, 2)
                vs.append(np.rint(a * (1 << frac_bits)).astype(np.int64))
                vp.append(vp[-1] + a.shape[0])
            lp.append(len(vp) - 1)
        off.append(off[-1] + len(per))
    v = np.concatenate(vs) if vs else np.zeros((0, 2), np.int64)
    if v.size and np.abs(v).max() >= 1 << 24:
        raise ValueError("rasterize_polygons: coordinates must stay below 2^24 in fixed-point units")
    cap = _capacity(crossing_capacity, _crossings(v, np.asarray(vp), H, frac_bits), "crossing_capacity")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    _lib.require_hip(dev, "rasterize_polygons")
    mk = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(dev)  # noqa: E731
    return _fill(dev, mk(lp, torch.int64), mk(vp, torch.int64), mk(v, torch.int32).reshape(-1, 2), mk(off, torch.int64), len(polygons), H, W,
                 frac_bits, cap, return_status)


def _fill(dev, loop_ptr, vertex_ptr, vertices, offsets, B, H, W, frac_bits, cap, return_status):
    _lib.require_hip(dev, "rasterize_polygons")
    labels = torch.empty((B, H, W), device=dev, dtype=torch.int32)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.call("mgu_polygons_to_labels", dev, loop_ptr, vertex_ptr, vertices, vertex_ptr.numel() - 1, vertices.shape[0], offsets,
              loop_ptr.numel() - 1, B, H, W, frac_bits, cap, labels, status)
    out = (labels, offsets[1:] - offsets[:-1], offsets)
    return out + (status,) if return_status else out


# ---- annotations as an ObjectTable -----------------------------------------------------------------------------------------------------
def objects_from_annotations(labels: torch.Tensor, counts: torch.Tensor, offsets: torch.Tensor, class_id) -> ObjectTable:
    """The ObjectTable of a label map built from annotations (labels_from_runs, rasterize_polygons): class_id gives the class of every
    object, batch-wide in row order (a sequence or an int64 tensor of offsets[B] entries).  area, bbox and sums come from
    mgu_object_stats on the class map gathered through the labels, so they describe the pixels an object keeps where annotations
    overlap.  object_overlaps(gt, pred), match_masks, panoptic_totals and border_weights then take COCO ground truth as they take
    connected_components' tables.  Synchronises once, as connected_components does, to size the per-object arrays."""
    _lib.require_hip(labels, "objects_from_annotations")
    dev = labels.device
    cls = torch.as_tensor(class_id, dtype=torch.int64).to(dev).reshape(-1)
    B = labels.shape[0]
    if cls.numel():
        row = (offsets[:B].view(B, 1, 1) + labels.to(torch.int64) - 1).clamp(0, cls.numel() - 1)
        cmap = torch.where(labels > 0, cls[row], torch.zeros((), device=dev, dtype=torch.int64)).contiguous()
    else:
        cmap = torch.zeros(labels.shape, device=dev, dtype=torch.int64)
    table = _table(labels.contiguous(), counts, offsets, cmap, 0, 0)
    if table.class_id.numel() != cls.numel():
        raise ValueError(f"objects_from_annotations: {cls.numel()} classes for {table.class_id.numel()} objects")
    table.class_id = cls          # an object hidden under larger labels has no pixel to read its class from
    return table
