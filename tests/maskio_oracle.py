"""Plain numpy, sequential statements of what csrc/maskio.hip computes: the runs of a label map in COCO's
column-major order, the label map of a run table, the crack-edge outlines of every object and the even-odd polygon fill.  Written
for reading; the GPU tests hold the kernels bitwise equal to these.  Every function takes the arrays in the device's own layout.

The keyword arguments named `mutant_*` switch ONE rule to a plausible mistake; tests/test_maskio_host.py asserts that every such
mutant fails a named case of tests/maskio_cases.py, so that the cases are known to see those mistakes."""
from collections import defaultdict

import numpy as np


def object_masks(labels, offsets):
    """yield (batch-wide row i, image b, bool mask (H, W)) for every object of the batch; a label outside [1, n_b] is no object"""
    for b in range(labels.shape[0]):
        for k in range(1, int(offsets[b + 1] - offsets[b]) + 1):
            yield int(offsets[b]) + k - 1, b, labels[b] == k


# ---- runs ----------------------------------------------------------------------------------------------------------------------------
def mask_runs(mask, mutant_row_major=False, mutant_no_wrap=False):
    """(starts, lengths) of the maximal intervals of consecutive positions p = x * H + y that the mask covers"""
    H = mask.shape[0]
    flat = mask.flatten(order="C" if mutant_row_major else "F").astype(np.int8)
    d = np.diff(np.concatenate(([0], flat, [0])))
    starts, ends = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    if mutant_no_wrap:   # a run cut at every column end
        cut = [(max(s, c), min(e, c + H)) for s, e in zip(starts, ends) for c in range(s // H * H, e, H)]
        starts, ends = np.array([s for s, _ in cut], np.int64), np.array([e for _, e in cut], np.int64)
    return starts, ends - starts


def encode(labels, offsets, **mutant):
    """(run_ptr int64 (N + 1), run_start int32, run_length int32): CSR by object, ascending start inside an object"""
    ptr, start, length = [0], [], []
    for _i, _b, mask in object_masks(labels, offsets):
        s, n = mask_runs(mask, **mutant)
        start += s.tolist()
        length += n.tolist()
        ptr.append(len(start))
    return np.array(ptr, np.int64), np.array(start, np.int32), np.array(length, np.int32)


def decode(run_ptr, run_start, run_length, offsets, B, H, W, mutant_smallest_wins=False):
    """(labels int32 (B, H, W), status): zeros, then every valid run paints its object's label; the largest label wins"""
    labels, status = np.zeros((B, H, W), np.int32), 0
    for b in range(B):
        flat = np.zeros(H * W, np.int32)   # column-major
        for i in range(int(offsets[b]), int(offsets[b + 1])):
            k = i - int(offsets[b]) + 1
            for j in range(int(run_ptr[i]), int(run_ptr[i + 1])):
                s, n = int(run_start[j]), int(run_length[j])
                if s < 0 or n < 1 or s + n > H * W:
                    status |= 1
                    continue
                seg = flat[s:s + n]
                seg[...] = np.where((seg == 0) | (seg > k), k, seg) if mutant_smallest_wins else np.maximum(seg, k)
        labels[b] = flat.reshape(W, H).T
    return labels, status


def coco_counts(starts, lengths, HW):
    """COCO's counts of one mask: zeros first, alternating, a trailing zero-run only when the mask does not end the image"""
    counts, pos = [], 0
    for s, n in zip(starts.tolist(), lengths.tolist()):
        counts += [s - pos, n]
        pos = s + n
    return counts + ([HW - pos] if pos < HW else [])


# ---- outlines --------------------------------------------------------------------------------------------------------------------------
CORNER = [(0, 0), (1, 0), (1, 1), (0, 1)]            # side s of pixel (x, y) starts at (x, y) + CORNER[s] and ends at + CORNER[s + 1]
ACROSS = [(0, -1), (1, 0), (0, 1), (-1, 0)]          # the pixel across side s


def mask_loops(mask, connectivity, mutant_wrong_turn=False, mutant_start_at_leader=False):
    """The loops of one object: a list of (vertices [(x, y), ...], area2), by ascending leader (the loop's smallest edge id)."""
    H, W = mask.shape
    inside = lambda x, y: 0 <= x < W and 0 <= y < H and bool(mask[y, x])  # noqa: E731
    edges, leaving = {}, defaultdict(list)           # id -> (start point, end point); start point -> ids
    for y, x in np.argwhere(mask):
        for s in range(4):
            if not inside(x + ACROSS[s][0], y + ACROSS[s][1]):
                e = (y * W + x) * 4 + s
                a, b = CORNER[s], CORNER[(s + 1) % 4]
                edges[e] = ((x + a[0], y + a[1]), (x + b[0], y + b[1]))
                leaving[edges[e][0]].append(e)
    succ = {}
    for e, (_, end) in edges.items():
        out = leaving[end]
        if len(out) == 1:
            succ[e] = out[0]
        else:                                        # two pixels of the object meet diagonally here
            right = e // 4 * 4 + (e % 4 + 1) % 4     # the next side of the same pixel
            left = [o for o in out if o != right][0]
            succ[e] = (right if connectivity == 1 else left) if not mutant_wrong_turn else (left if connectivity == 1 else right)
    assert sorted(succ.values()) == sorted(edges)    # a permutation of the object's edges
    loops, seen = [], set()
    for leader in sorted(edges):
        if leader in seen:
            continue
        cycle, e = [], leader
        while e not in seen:
            seen.add(e)
            cycle.append(e)
            e = succ[e]
        # a vertex: the start point of an edge whose predecessor has another direction (the side number is the direction)
        corner = [cycle[j] % 4 != cycle[j - 1] % 4 for j in range(len(cycle))]
        if mutant_start_at_leader:
            corner[0] = True
        first = corner.index(True)                                      # the first corner at or after the leader's start point
        order, keep = cycle[first:] + cycle[:first], corner[first:] + corner[:first]
        v = [edges[e][0] for e, k in zip(order, keep) if k]
        area2 = sum(v[j][0] * v[(j + 1) % len(v)][1] - v[(j + 1) % len(v)][0] * v[j][1] for j in range(len(v)))
        loops.append((v, area2))
    return loops


def outlines(labels, offsets, connectivity, **mutant):
    """(loop_ptr int64 (N + 1), vertex_ptr int64 (loops + 1), vertices int32 (V, 2), loop_area2 int64 (loops))"""
    lp, vp, vs, a2 = [0], [0], [], []
    for _i, _b, mask in object_masks(labels, offsets):
        for v, area2 in mask_loops(mask, connectivity, **mutant):
            vs += v
            vp.append(len(vs))
            a2.append(area2)
        lp.append(len(a2))
    return np.array(lp, np.int64), np.array(vp, np.int64), np.array(vs, np.int32).reshape(-1, 2), np.array(a2, np.int64)


# ---- polygon fill ----------------------------------------------------------------------------------------------------------------------
def loops_cover(loops, H, W, frac_bits, mutant_strict=False):
    """bool (H, W): the pixels whose centre an odd number of the loops' edges count for.  loops: int arrays (n, 2) in fixed point.
    Doubled units: X = 2 v, Cx = (2x + 1) 2^f, Cy = (2y + 1) 2^f; the edge (x0, y0) -> (x1, y1) counts iff (y0 <= Cy) != (y1 <= Cy)
    and, ordered so that y0 < y1, x0 (y1 - y0) + (x1 - x0)(Cy - y0) < Cx (y1 - y0)."""
    S = 1 << frac_bits
    cx = ((2 * np.arange(W, dtype=np.int64) + 1) * S)[None, :]
    cy = ((2 * np.arange(H, dtype=np.int64) + 1) * S)[:, None]
    odd = np.zeros((H, W), bool)
    for loop in loops:
        v = 2 * np.asarray(loop, np.int64).reshape(-1, 2)
        for j in range(len(v)):
            (x0, y0), (x1, y1) = v[j], v[(j + 1) % len(v)]
            if y0 > y1:
                x0, y0, x1, y1 = x1, y1, x0, y0
            spans = ((y0 < cy) != (y1 < cy)) if mutant_strict else ((y0 <= cy) != (y1 <= cy))
            odd ^= spans & (x0 * (y1 - y0) + (x1 - x0) * (cy - y0) < cx * (y1 - y0))
    return odd


def fill(loop_ptr, vertex_ptr, vertices, offsets, B, H, W, frac_bits=0, mutant_smallest_wins=False, **mutant):
    """labels int32 (B, H, W): zeros, then every object paints its label over the pixels its loops cover; the largest label wins"""
    labels = np.zeros((B, H, W), np.int32)
    for b in range(B):
        for i in range(int(offsets[b]), int(offsets[b + 1])):
            k = i - int(offsets[b]) + 1
            loops = [vertices[vertex_ptr[l]:vertex_ptr[l + 1]] for l in range(int(loop_ptr[i]), int(loop_ptr[i + 1]))]
            cover = loops_cover(loops, H, W, frac_bits, **mutant)
            lab = labels[b]
            if mutant_smallest_wins:
                lab[cover & ((lab == 0) | (lab > k))] = k
            else:
                lab[cover] = np.maximum(lab[cover], k)
    return labels


def polygon_table(per_image, frac_bits=0):
    """per image a list of objects, an object a list of loops, a loop a sequence of (x, y) in pixel units ->
    (loop_ptr, vertex_ptr, vertices int32 in fixed point, offsets)"""
    lp, vp, vs, off = [0], [0], [], [0]
    for per in per_image:
        for loops in per:
            for loop in loops:
                a = np.rint(np.asarray(loop, np.float64).reshape(-1, 2) * (1 << frac_bits)).astype(np.int32)
                vs.append(a)
                vp.append(vp[-1] + len(a))
            lp.append(len(vp) - 1)
        off.append(off[-1] + len(per))
    v = np.concatenate(vs) if vs else np.zeros((0, 2), np.int32)
    return np.array(lp, np.int64), np.array(vp, np.int64), v.reshape(-1, 2), np.array(off, np.int64)
