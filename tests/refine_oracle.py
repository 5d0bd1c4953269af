"""numpy oracle of mgu_refine_probs (include/mgunet.h states the definition): int64 throughout, one shifted-slice pass per tap, and a
per-pixel triple loop that tests/test_refine_host.py holds it against.  The tables are computed here on their own, from the formulas of
the definition, so that mgunet.bilateral_tables has something to be compared with."""
import math

import numpy as np

RANGE = 1024


def tables(radius, sigma_space, sigma_color):
    """(space_lut int64 (r+1, r+1), range_lut int64 (1024,), shift) in float64, term by term"""
    r = int(radius)
    space = np.zeros((r + 1, r + 1), np.int64)
    for a in range(r + 1):
        for b in range(r + 1):
            space[a, b] = int(np.rint(256.0 * math.exp(-(a * a + b * b) / (2.0 * sigma_space * sigma_space))))
    top = math.ceil(12.5 * sigma_color * sigma_color)
    shift = 8
    for s in range(9):
        if (top >> s) <= RANGE - 1:
            shift = s
            break
    rng = np.array([int(np.rint(256.0 * math.exp(-float(k << shift) / (2.0 * sigma_color * sigma_color)))) for k in range(RANGE)], np.int64)
    return space, rng, shift


def quantise(x):
    """q0: rint(clamp(x, 0, 1) * 65535) with the product in float32, NaN -> 0; int64 array of x's shape"""
    x = np.asarray(x, np.float32)
    v = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1))).astype(np.float32)
    return np.rint(v * np.float32(65535)).astype(np.int64)


def first_max(q):
    """(..., C) -> the first maximal class"""
    return np.argmax(q, axis=-1).astype(np.int64)          # numpy returns the first occurrence


def _batched(x, guide):
    x = np.asarray(x, np.float32)
    guide = np.asarray(guide)
    assert guide.dtype == np.uint8
    if x.ndim == 3:
        x = x[None]
    if guide.ndim == 2:
        guide = guide[:, :, None]
    if guide.ndim == 3 and x.shape[:3] != guide.shape[:3]:
        guide = guide[None]
    assert guide.shape[:3] == x.shape[:3] and guide.shape[3] in (1, 3), (x.shape, guide.shape)
    return x, guide.astype(np.int64)


def iterate(q, guide, space, rng, shift):
    """one iteration on (B, H, W, C) int64 planes: a pass over shifted slices per tap"""
    B, H, W, C = q.shape
    r = space.shape[0] - 1
    num = np.zeros(q.shape, np.int64)
    den = np.zeros((B, H, W), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)      # pixels p with p + d inside
            if ys >= ye or xs >= xe:
                continue
            a = guide[:, ys:ye, xs:xe]
            b = guide[:, ys + dy:ye + dy, xs + dx:xe + dx]
            d2 = ((a - b) ** 2).sum(-1)
            w = (space[abs(dy), abs(dx)] * rng[np.minimum(d2 >> shift, RANGE - 1)] + 128) >> 8
            den[:, ys:ye, xs:xe] += w
            num[:, ys:ye, xs:xe] += w[..., None] * q[:, ys + dy:ye + dy, xs + dx:xe + dx]
    assert int(num.max(initial=0)) < 2 ** 32 and int(den.min(initial=1)) >= 1
    return (num + (den >> 1)[..., None]) // den[..., None]


def iterate_brute(q, guide, space, rng, shift):
    """the same by a loop over pixels, taps and classes"""
    B, H, W, C = q.shape
    r = space.shape[0] - 1
    out = np.zeros(q.shape, np.int64)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                num, den = [0] * C, 0
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        yy, xx = y + dy, x + dx
                        if yy < 0 or yy >= H or xx < 0 or xx >= W:
                            continue
                        d2 = sum((int(guide[b, y, x, g]) - int(guide[b, yy, xx, g])) ** 2 for g in range(guide.shape[3]))
                        w = (int(space[abs(dy), abs(dx)]) * int(rng[min(d2 >> shift, RANGE - 1)]) + 128) >> 8
                        den += w
                        for k in range(C):
                            num[k] += w * int(q[b, yy, xx, k])
                for k in range(C):
                    out[b, y, x, k] = (num[k] + (den >> 1)) // den
    return out


def refine_q(q0, guide, space, rng, shift, iterations, step=iterate):
    q = q0
    for _ in range(int(iterations)):
        q = step(q, guide, space, rng, shift)
    return q


def refine(x, guide, space, rng, shift, iterations, step=iterate):
    """x: float32 (B, H, W, C) (or (H, W, C)) probabilities; guide uint8 (B, H, W, G) / (H, W, G) / (H, W).
    -> (probs float32 (B, H, W, C), labels int64 (B, H, W), conf float32 (B, H, W), changed int64 (B,), q int64)"""
    x, guide = _batched(x, guide)
    space, rng = np.asarray(space, np.int64).reshape(-1), np.asarray(rng, np.int64)
    n1 = int(round(math.sqrt(space.size)))
    space = space.reshape(n1, n1)
    q0 = quantise(x)
    q = refine_q(q0, guide, space, rng, int(shift), iterations, step)
    labels = first_max(q)
    probs = (q.astype(np.float32) / np.float32(65535)).astype(np.float32)
    conf = np.take_along_axis(probs, labels[..., None], -1)[..., 0]
    changed = (labels != first_max(q0)).reshape(labels.shape[0], -1).sum(1).astype(np.int64)
    return probs, labels, conf, changed, q


# ---- the snap scenario of the issue: an outline three pixels off a colour edge ---------------------------------------------------------
def snap_scene(one_hot, seed=0):
    """(probabilities float32 (48, 48, 2), guide uint8 (48, 48, 3)): the guide is 60 left of column 24 and 180 from it on, plus uniform
    noise in [-4, 4]; class 1's probability is a logistic ramp centred on column 27 (scale 2), or its one-hot version: class 1 from the
    ramp's centre, column 27, on"""
    rs = np.random.RandomState(seed)
    base = np.where(np.arange(48) < 24, 60, 180)[None, :, None]
    guide = (base + rs.randint(-4, 5, (48, 48, 3))).astype(np.uint8)
    p1 = 1.0 / (1.0 + np.exp(-(np.arange(48, dtype=np.float64) - 27.0) / 2.0))
    if one_hot:
        p1 = (p1 >= 0.5).astype(np.float64)
    p1 = np.broadcast_to(p1[None, :], (48, 48))
    return np.stack([1.0 - p1, p1], -1).astype(np.float32), guide


def outline_columns(labels):
    """per row of a two-class (H, W) map that is 0 then 1: the column of the first 1; asserts that form"""
    cols = []
    for row in np.asarray(labels):
        k = int(np.argmax(row))
        assert row[k] == 1 and not row[:k].any() and row[k:].all(), row
        cols.append(k)
    return cols
