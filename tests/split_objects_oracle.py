"""numpy oracle of mgunet.distance_transform and mgunet.split_objects, shared by the split tests.  It follows the definitions of
include/mgunet.h (mgu_split_objects) step by step, all in integers:
  1. d2(p): the smallest |p - q|^2 over the pixels q of the image whose label differs from p's (background included, pixels outside
     the image excluded); D2_NONE = 2^30 when there is none; 0 on background.
  2. seeds: d2(p) >= min_radius_sq and d2(p) >= d2(q) for every q of p's label within Chebyshev distance r.
  3. zone map: Z(p) = label(p) when a seed of p's label lies within Chebyshev distance h = (r + 1) // 2, else 0; the seed groups are
     the 8-connected same-value components of Z.
  4. a pixel of a component that has seeds goes to the group of the seed s of its component minimising (|p - s|^2 - d2(s), index of
     s); a component without seeds stays whole.
  5. objects are numbered in raster order of their first pixel; objects under min_area pixels are dropped and the rest renumbered.
Clarity over speed: the distances are explicit minima over all pixels."""
import numpy as np

import objects_oracle as OO

D2_NONE = 1 << 30


def d2(labels):
    """int32 (H, W): squared distance of every foreground pixel to the nearest pixel holding another label."""
    labels = np.asarray(labels)
    H, W = labels.shape
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((H, W), np.int64)
    for k in np.unique(labels):
        if k == 0:
            continue
        mine, other = labels == k, labels != k
        if not other.any():
            out[mine] = D2_NONE
            continue
        py, px, qy, qx = ys[mine], xs[mine], ys[other], xs[other]
        best = np.empty(py.size, np.int64)
        for i in range(0, py.size, 256):   # the explicit minimum, 256 pixels at a time
            best[i:i + 256] = ((py[i:i + 256, None] - qy[None]) ** 2 + (px[i:i + 256, None] - qx[None]) ** 2).min(1)
        out[mine] = best
    return out.astype(np.int32)


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside the image."""
    H, W = a.shape
    b = np.full_like(a, fill)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return b


def seeds(labels, dist, r, min_radius_sq):
    """bool (H, W): the seed pixels."""
    labels, dist = np.asarray(labels), np.asarray(dist, np.int64)
    ok = (labels != 0) & (dist >= min_radius_sq)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ok &= ~((_shifted(labels, dy, dx, 0) == labels) & (_shifted(dist, dy, dx, 0) > dist))
    return ok


def zone_map(labels, seed, r):
    labels = np.asarray(labels)
    h = (r + 1) // 2
    sl = np.where(seed, labels, 0)
    z = np.zeros_like(labels)
    for dy in range(-h, h + 1):
        for dx in range(-h, h + 1):
            z = np.where((labels != 0) & (_shifted(sl, dy, dx, 0) == labels), labels, z)
    return z


def split(labels, min_distance=5, min_radius_sq=9, min_area=0, seed_order=None, dist=None):
    """One (H, W) label map -> dict(d2, seeds, labels, count).  seed_order: a function permuting each component's seed list (the
    result must not depend on it).  dist: d2(labels), when the caller has it already."""
    labels = np.asarray(labels).astype(np.int64)
    H, W = labels.shape
    dist = d2(labels) if dist is None else dist
    seed = seeds(labels, dist, min_distance, min_radius_sq)
    groups = OO.label(zone_map(labels, seed, min_distance), 2)   # 1..G; every seed pixel lies in its own zone
    prov = np.zeros((H, W), np.int64)
    G = int(groups.max()) if groups.size else 0
    lin = np.arange(H * W).reshape(H, W)
    for j, k in enumerate(np.unique(labels)):
        if k == 0:
            continue
        mine = labels == k
        sy, sx = np.nonzero(mine & seed)
        if sy.size == 0:
            prov[mine] = G + 1 + j   # no seed: the component stays one object
            continue
        if seed_order is not None:
            perm = seed_order(sy.size)
            sy, sx = sy[perm], sx[perm]
        py, px = np.nonzero(mine)
        cost = (py[:, None] - sy[None]) ** 2 + (px[:, None] - sx[None]) ** 2 - dist[sy, sx].astype(np.int64)[None]
        key = cost * (H * W) + lin[sy, sx][None]   # (cost, seed index) in lexicographic order: cost is an integer, index < H*W
        best = key.argmin(1)
        prov[mine] = groups[sy[best], sx[best]]
    out = np.zeros((H, W), np.int32)
    ids, first = np.unique(prov.reshape(-1), return_index=True)
    n = 0
    for i in ids[np.argsort(first)]:
        if i == 0:
            continue
        m = prov == i
        if m.sum() >= min_area:
            n += 1
            out[m] = n
    return {"d2": dist, "seeds": seed, "labels": out, "count": n}


def split_batch(labels, min_distance=5, min_radius_sq=9, min_area=0, dist=None):
    """(B, H, W) -> d2 int32 (B, H, W), seeds bool, labels int32, counts int64 (B), offsets int64 (B + 1)."""
    res = [split(m, min_distance, min_radius_sq, min_area, dist=None if dist is None else dist[b]) for b, m in enumerate(np.asarray(labels))]
    counts = np.array([r["count"] for r in res], np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    stack = lambda key, dt: np.stack([r[key] for r in res]).astype(dt) if res else np.zeros(np.asarray(labels).shape, dt)  # noqa: E731
    return stack("d2", np.int32), stack("seeds", bool), stack("labels", np.int32), counts, offsets


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
def disc(shape, cy, cx, R):
    ys, xs = np.mgrid[0:shape[0], 0:shape[1]]
    return (ys - cy) ** 2 + (xs - cx) ** 2 <= R * R


def ellipse(shape, cy, cx, a, b, angle):
    ys, xs = np.mgrid[0:shape[0], 0:shape[1]]
    u = (xs - cx) * np.cos(angle) + (ys - cy) * np.sin(angle)
    v = -(xs - cx) * np.sin(angle) + (ys - cy) * np.cos(angle)
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


def two_discs(sep, shape=(96, 128), R=20):
    """One component of two radius-R discs whose centres lie `sep` pixels apart on the middle row; returns (mask, centres)."""
    cy, c0 = shape[0] // 2, (shape[1] - sep) // 2
    return disc(shape, cy, c0, R) | disc(shape, cy, c0 + sep, R), ((cy, c0), (cy, c0 + sep))


def touching_pairs(n=3, R=9, step=11, shape=(48, 160)):
    """n pairs of overlapping radius-R discs, the second `step` pixels right of and below the first, in one class-1 map: as one
    blob a pair's box overlaps either disc's box with IoU (2R + 1)^2 / (2R + 1 + step)^2 < 1/2.  Returns (class map int64, the 2n
    discs' boxes [xmin, ymin, xmax, ymax))."""
    m = np.zeros(shape, np.int64)
    boxes = []
    for i in range(n):
        for cy, cx in ((14, 16 + 50 * i), (14 + step, 16 + 50 * i + step)):
            m[disc(shape, cy, cx, R)] = 1
            boxes.append([cx - R, cy - R, cx + R + 1, cy + R + 1])
    return m, boxes


def touching_pairs_expected(n=3, smooth=1e-6):
    """yield_estimation_metrics of touching_pairs(n) once the pairs are split: 2n objects on both sides, every one matched."""
    return {"count_accuracy_perc": 100.0, "yield_estimation_error_perc": 0.0, "object_matching_rate_perc": (2 * n / (2 * n + smooth)) * 100,
            "occlusion_robustness_perc": -1.0, "total_gt_count_sum": 2 * n, "total_pred_count_sum": 2 * n}
