"""numpy / scipy oracle of mgunet.boundary_tables, shared by the boundary tests.  It restates the definitions of include/mgunet.h
(mgu_boundary_tables) with scipy's exact Euclidean distance transform instead of the device's column and row passes:
  0. classes 1 .. num_classes - 1 are foreground; every other value reads as background (0), on both sides.
  1. boundary of class c in a map: the pixels of class c with a 4-neighbour inside the image holding another value.
  2. surface distance, direction 0: for every boundary pixel of the prediction, the squared distance to the nearest boundary pixel of
     the same class in the target (np.rint(distance_transform_edt(~sites) ** 2)); unmatched when the target has none.  Direction 1 is
     the converse.  Histogram bins 0 .. max_d2 and one overflow bin (d2 > max_d2 and the unmatched); n, n_unmatched, the max and the
     sum of math.isqrt(d2 << 32) over the matched pixels.
  3. band of class c in a map: its pixels whose squared distance to the nearest pixel of the image holding another value (the EDT of the
     class mask) is <= band_r2; [|P & G|, |P|, |G|].
Every function takes one (H, W) image but tables(), which takes a batch."""
import math

import numpy as np
from scipy import ndimage

D2_NONE = 1 << 30   # MGU_D2_NONE: the image holds no other value


def radius_sq(radius) -> int:
    """floor(radius^2), as mgunet.boundary_tables squares max_distance and band_radius"""
    return int(math.floor(float(radius) ** 2 + 1e-9))


def default_band_r2(H, W) -> int:
    return max(1, radius_sq(0.02 * math.hypot(H, W)))


def normalise(m, num_classes):
    m = np.asarray(m).astype(np.int64)
    return np.where((m >= 1) & (m < num_classes), m, 0)


def boundary(m, c):
    """bool (H, W): the pixels of class c with a 4-neighbour inside the image holding another value"""
    other = m != c
    nb = np.zeros(m.shape, bool)
    nb[1:] |= other[:-1]
    nb[:-1] |= other[1:]
    nb[:, 1:] |= other[:, :-1]
    nb[:, :-1] |= other[:, 1:]
    return (m == c) & nb


def mask_d2(mask):
    """int64 (H, W): the squared distance of every pixel of the mask to the nearest pixel outside it (inside the image), D2_NONE when the
    mask is the whole image, 0 outside the mask"""
    if mask.all():
        return np.full(mask.shape, D2_NONE, np.int64)
    return np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)


def site_d2(sites):
    """int64 (H, W): the squared distance of every pixel to the nearest site; None when there is no site"""
    if not sites.any():
        return None
    return np.rint(ndimage.distance_transform_edt(~sites) ** 2).astype(np.int64)


def directed(src_sites, dst_sites, max_d2):
    """(histogram (max_d2 + 2), [n, n_unmatched, max, sum of isqrt(d2 << 32)]) of the source sites against the destination's"""
    hist, n = np.zeros(max_d2 + 2, np.int64), int(src_sites.sum())
    d = site_d2(dst_sites)
    if d is None:
        hist[max_d2 + 1] = n
        return hist, [n, n, 0, 0]
    d = d[src_sites]
    hist += np.bincount(np.minimum(d, max_d2 + 1), minlength=max_d2 + 2)
    return hist, [n, 0, int(d.max()) if n else 0, sum(math.isqrt(int(v) << 32) for v in d)]


def tables(pred, target, num_classes, max_d2, band_r2):
    """(hist (B, K, 2, max_d2 + 2), stats (B, K, 2, 4), band (B, K, 3)), int64, of class maps (B, H, W)"""
    pred, target = np.asarray(pred), np.asarray(target)
    B, K = pred.shape[0], num_classes - 1
    hist, stats, band = np.zeros((B, K, 2, max_d2 + 2), np.int64), np.zeros((B, K, 2, 4), np.int64), np.zeros((B, K, 3), np.int64)
    for b in range(B):
        p, g = normalise(pred[b], num_classes), normalise(target[b], num_classes)
        if p.size == 0:
            continue
        for c in range(1, num_classes):
            dp, dg = boundary(p, c), boundary(g, c)
            hist[b, c - 1, 0], stats[b, c - 1, 0] = directed(dp, dg, max_d2)
            hist[b, c - 1, 1], stats[b, c - 1, 1] = directed(dg, dp, max_d2)
            bp, bg = (p == c) & (mask_d2(p == c) <= band_r2), (g == c) & (mask_d2(g == c) <= band_r2)
            band[b, c - 1] = [(bp & bg).sum(), bp.sum(), bg.sum()]
    return hist, stats, band


def argmax_first(logits_nchw):
    """first maximal class of (B, C, H, W) logits"""
    return np.argmax(np.asarray(logits_nchw), axis=1).astype(np.int64)


# ---- brute force, for the oracle's own test -----------------------------------------------------------------------------------------
def brute_tables(pred, target, num_classes, max_d2, band_r2):
    """tables() by literal loops: 4-neighbour tests pixel by pixel and all-pairs distances (tiny maps only)"""
    pred, target = np.asarray(pred), np.asarray(target)
    B, H, W = pred.shape
    K = num_classes - 1
    hist, stats, band = np.zeros((B, K, 2, max_d2 + 2), np.int64), np.zeros((B, K, 2, 4), np.int64), np.zeros((B, K, 3), np.int64)

    def cls(m, y, x):
        v = int(m[y, x])
        return v if 1 <= v < num_classes else 0

    def sites(m, c):
        out = []
        for y in range(H):
            for x in range(W):
                if cls(m, y, x) == c and any(0 <= y + dy < H and 0 <= x + dx < W and cls(m, y + dy, x + dx) != c
                                             for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0))):
                    out.append((y, x))
        return out

    def in_band(m, c):
        other = [(y, x) for y in range(H) for x in range(W) if cls(m, y, x) != c]
        return {(y, x) for y in range(H) for x in range(W)
                if cls(m, y, x) == c and other and min((y - v) ** 2 + (x - u) ** 2 for v, u in other) <= band_r2}

    for b in range(B):
        for c in range(1, num_classes):
            s = [sites(pred[b], c), sites(target[b], c)]
            for d in (0, 1):
                src, dst = s[d], s[1 - d]
                row = stats[b, c - 1, d]
                row[0] = len(src)
                for y, x in src:
                    if not dst:
                        row[1] += 1
                        hist[b, c - 1, d, max_d2 + 1] += 1
                        continue
                    d2 = min((y - v) ** 2 + (x - u) ** 2 for v, u in dst)
                    hist[b, c - 1, d, min(d2, max_d2 + 1)] += 1
                    row[2] = max(row[2], d2)
                    row[3] += math.isqrt(d2 << 32)
            bp, bg = in_band(pred[b], c), in_band(target[b], c)
            band[b, c - 1] = [len(bp & bg), len(bp), len(bg)]
    return hist, stats, band


# ---- scenes shared by the host and the device tests ---------------------------------------------------------------------------------
def blob_pair(shape, C, seed, junk=True):
    """(logit planes (B, C, H, W) float32 with ties, prediction class map, target class map): the argmax of quantised smooth noise and of a
    perturbed copy of the same noise, with -100 and out-of-range values sprinkled on both maps (not on the planes' argmax)"""
    B, H, W = shape
    rng = np.random.default_rng(seed)
    x = np.stack([[ndimage.gaussian_filter(rng.standard_normal((H, W)), 2.5, mode="constant") for _ in range(C)] for _ in range(B)])
    x[:, 0] += 0.02
    y = x + 0.25 * np.stack([[ndimage.gaussian_filter(rng.standard_normal((H, W)), 1.5, mode="constant") for _ in range(C)] for _ in range(B)])
    q = lambda a: (np.round(a * 16) / 16 + (rng.random(a.shape) < 0.03) * rng.integers(-1, 2, a.shape) * 0.5).astype(np.float32)  # noqa: E731
    planes = q(x)
    pred, target = argmax_first(planes), argmax_first(q(y))
    if junk:
        for m in (pred, target):
            u = rng.random(m.shape)
            m[u < 0.01] = -100
            m[(u >= 0.01) & (u < 0.02)] = C + 3
    return planes, pred, target


def two_squares():
    """the hand scene: an 8 x 8 square in a 20 x 30 image against the same square 3 columns to the right"""
    p, g = np.zeros((1, 20, 30), np.int64), np.zeros((1, 20, 30), np.int64)
    p[0, 6:14, 8:16] = 1
    g[0, 6:14, 11:19] = 1
    return p, g
