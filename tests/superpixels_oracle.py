"""numpy oracle of the superpixel-graph stages (include/mgunet.h, "superpixel graphs"; mgunet/superpixels.py): integer SLIC, connected and
merged regions, region adjacency, node features and region pooling.  Everything the device computes is integer arithmetic or one
double expression of integers, so the GPU tests compare bit for bit.  The colour tables are mgunet.lab_tables(), the single host
description both sides read.  tests/test_superpixels_host.py pins this file against brute-force loops, scipy and hand-made cases."""
import numpy as np

from mgunet.superpixels import lab_tables


def rgb_to_lab_q(rgb, tables=None):
    """uint8 (..., 3) -> int64 (..., 3) quarter-unit CIELAB [L, a, b]"""
    LIN, M, F = lab_tables() if tables is None else tables
    lin = LIN.astype(np.int64)[np.asarray(rgb)]
    xyz = (lin @ M.astype(np.int64).T + 2048) >> 12
    f = F.astype(np.int64)[xyz]
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    return np.stack([(116 * fy - 16384 + 128) >> 8, (500 * (fx - fy) + 128) >> 8, (200 * (fy - fz) + 128) >> 8], axis=-1)


def slic_grid(H, W, S):
    return -(-W // S), -(-H // S)


def slic_init_centres(lab, S):
    """int64 (gy * gx, 6) [x, y, L, a, b, n = 0] of one image's Lab (H, W, 3)"""
    H, W = lab.shape[:2]
    gx, gy = slic_grid(H, W, S)
    cx = np.minimum(np.arange(gx) * S + S // 2, W - 1)
    cy = np.minimum(np.arange(gy) * S + S // 2, H - 1)
    yy, xx = np.meshgrid(cy, cx, indexing="ij")
    cen = np.zeros((gy * gx, 6), np.int64)
    cen[:, 0], cen[:, 1] = xx.ravel(), yy.ravel()
    cen[:, 2:5] = lab[yy.ravel(), xx.ravel()]
    return cen


def slic_assign(lab, cen, S, mq):
    """one assignment pass: int64 (H, W) labels; candidates in ascending k, np.argmin keeps the first minimum (ties to the smaller k)"""
    H, W = lab.shape[:2]
    gx, gy = slic_grid(H, W, S)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    i, j = y // S, x // S
    Ds, ks = [], []
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ii, jj = i + di, j + dj
            ok = (ii >= 0) & (ii < gy) & (jj >= 0) & (jj < gx)
            k = np.where(ok, ii * gx + jj, 0)
            c = cen[k]
            dc2 = ((lab - c[..., 2:5]) ** 2).sum(-1)
            ds2 = (x - c[..., 0]) ** 2 + (y - c[..., 1]) ** 2
            Ds.append(np.where(ok, dc2 * (S * S) + (mq * mq) * ds2, np.iinfo(np.int64).max))
            ks.append(k)
    best = np.argmin(np.stack(Ds), axis=0)
    return np.take_along_axis(np.stack(ks), best[None], 0)[0]


def slic_update(lab, labels, cen):
    """centre update: floor((2 sum + n) / (2 n)) per value over the pixels of `labels`; n == 0 keeps the centre; [5] = n"""
    H, W = labels.shape
    K = cen.shape[0]
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    flat = labels.ravel()
    n = np.bincount(flat, minlength=K).astype(np.int64)
    out = cen.copy()
    has = n > 0
    for q, v in enumerate((x, y, lab[..., 0], lab[..., 1], lab[..., 2])):
        s = np.zeros(K, np.int64)
        np.add.at(s, flat, v.ravel().astype(np.int64))
        out[has, q] = (2 * s[has] + n[has]) // (2 * n[has])      # numpy's // on integers is floor division
    out[:, 5] = n
    return out


def slic(rgb, S, mq, T, tables=None):
    """uint8 (B, H, W, 3) -> (raw labels int32 (B, H, W), centres int32 (B, gx gy, 6) as the last pass read them)"""
    rgb = np.asarray(rgb)
    B, H, W = rgb.shape[:3]
    gx, gy = slic_grid(H, W, S)
    labels = np.zeros((B, H, W), np.int32)
    centres = np.zeros((B, gx * gy, 6), np.int32)
    for b in range(B):
        lab = rgb_to_lab_q(rgb[b], tables)
        cen = slic_init_centres(lab, S)
        for t in range(T):
            lb = slic_assign(lab, cen, S, mq)
            if t + 1 < T:
                cen = slic_update(lab, lb, cen)
        labels[b], centres[b] = lb, cen
    return labels, centres


def component_roots(raw):
    """(H, W) -> int64 (H, W): the smallest linear index of every pixel's 4-connected same-value component (min-label propagation
    with pointer jumping)"""
    H, W = raw.shape
    lab = np.arange(H * W, dtype=np.int64).reshape(H, W)
    eh, ev = raw[:, 1:] == raw[:, :-1], raw[1:] == raw[:-1]
    while True:
        new = lab.copy()
        new[:, 1:] = np.where(eh, np.minimum(new[:, 1:], lab[:, :-1]), new[:, 1:])
        new[:, :-1] = np.where(eh, np.minimum(new[:, :-1], lab[:, 1:]), new[:, :-1])
        new[1:] = np.where(ev, np.minimum(new[1:], lab[:-1]), new[1:])
        new[:-1] = np.where(ev, np.minimum(new[:-1], lab[1:]), new[:-1])
        new = np.minimum(new, new.ravel()[new])
        if np.array_equal(new, lab):
            return lab
        lab = new


def renumber(ids):
    """(H, W) ids -> int64 (H, W) 0..n-1 in raster order of each id's first pixel, and n"""
    _, first, inv = np.unique(ids.ravel(), return_index=True, return_inverse=True)
    rank = np.empty(first.size, np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return rank[inv].reshape(ids.shape), first.size


def pixel_edges(L):
    """every horizontally or vertically adjacent pixel pair of (H, W) L as two int64 arrays (the labels on either side)"""
    return (np.concatenate([L[:, :-1].ravel(), L[:-1].ravel()]).astype(np.int64),
            np.concatenate([L[:, 1:].ravel(), L[1:].ravel()]).astype(np.int64))


def merge_round(L, n, min_area):
    """one merge round on regions 0..n-1 numbered in raster order of first pixel: (new labels, new n, regions merged)"""
    area = np.bincount(L.ravel(), minlength=n)
    small = area < min_area
    p, q = pixel_edges(L)
    s, d = np.concatenate([p, q]), np.concatenate([q, p])          # both orientations of every pixel edge
    keep = (s != d) & small[s] & ~small[d]
    if not keep.any():
        return L, n, 0
    key, cnt = np.unique(s[keep] * n + d[keep], return_counts=True)
    ks, kd = key // n, key % n
    order = np.lexsort((kd, -cnt, ks))                              # per small region: most shared edges, then the smaller d
    ks, kd = ks[order], kd[order]
    firsts = np.r_[True, ks[1:] != ks[:-1]]
    target = np.arange(n)
    target[ks[firsts]] = kd[firsts]
    out, m = renumber(target[L])
    return out, m, int(firsts.sum())


def connect(raw, min_area, rounds, history=None):
    """int (B, H, W) raw labels -> (labels int32 (B, H, W), counts int64 (B), offsets int64 (B + 1)).  history: a list that receives
    per image [(labels, n, merged)] after the components and after every round."""
    raw = np.asarray(raw)
    B = raw.shape[0]
    labels = np.zeros(raw.shape, np.int32)
    counts = np.zeros(B, np.int64)
    for b in range(B):
        L, n = renumber(component_roots(raw[b]))
        steps = [(L, n, 0)]
        for _ in range(rounds):
            L, n, merged = merge_round(L, n, min_area)
            steps.append((L, n, merged))
        labels[b], counts[b] = L, n
        if history is not None:
            history.append(steps)
    return labels, counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def adjacency(labels, offsets, node_capacity):
    """-> (rowptr int32 (node_capacity + 1), col int32 (E), border int32 (E), status bit 2): both directions, rows by batch-wide
    node, columns ascending; labels outside [0, n_b) take no part; an image whose nodes pass node_capacity contributes nothing"""
    labels, offsets = np.asarray(labels), np.asarray(offsets)
    us, vs, status = [], [], 0
    for b in range(labels.shape[0]):
        o0, o1 = int(offsets[b]), int(offsets[b + 1])
        if o1 > node_capacity:
            status |= 2
            continue
        p, q = pixel_edges(labels[b])
        ok = (p != q) & (p >= 0) & (p < o1 - o0) & (q >= 0) & (q < o1 - o0)
        us += [o0 + p[ok], o0 + q[ok]]
        vs += [o0 + q[ok], o0 + p[ok]]
    u = np.concatenate(us) if us else np.zeros(0, np.int64)
    v = np.concatenate(vs) if vs else np.zeros(0, np.int64)
    big = node_capacity + 1
    key, cnt = np.unique(u * big + v, return_counts=True)
    rows, col = key // big, key % big
    rowptr = np.zeros(node_capacity + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), col.astype(np.int32), cnt.astype(np.int32), status


def _nodes(labels, offsets, node_capacity):
    """batch-wide node index of every pixel, -1 where the pixel belongs to no recorded node"""
    labels, offsets = np.asarray(labels).astype(np.int64), np.asarray(offsets)
    node = np.full(labels.shape, -1, np.int64)
    for b in range(labels.shape[0]):
        o0, o1 = int(offsets[b]), int(offsets[b + 1])
        if o1 <= node_capacity:
            node[b] = np.where((labels[b] >= 0) & (labels[b] < o1 - o0), o0 + labels[b], -1)
    return node


def _segment_sums(node, values, node_capacity):
    """exact int64 sums of values (N, K) per node (N,), nodes < 0 skipped -> (node_capacity, K)"""
    out = np.zeros((node_capacity, values.shape[1]), np.int64)
    ok = node >= 0
    if ok.any():
        order = np.argsort(node[ok], kind="stable")
        nd, vals = node[ok][order], values[ok][order]
        starts = np.flatnonzero(np.r_[True, nd[1:] != nd[:-1]])
        out[nd[starts]] = np.add.reduceat(vals, starts, axis=0)
    return out


def features(rgb, labels, offsets, node_capacity, tables=None):
    """-> (float32 (node_capacity, 8), stats int64 (node_capacity, 6) [area, sum x, sum y, sum L, sum a, sum b])"""
    rgb = np.asarray(rgb)
    B, H, W = rgb.shape[:3]
    node = _nodes(labels, offsets, node_capacity).ravel()
    lab = rgb_to_lab_q(rgb, tables).reshape(-1, 3)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    vals = np.concatenate([np.ones((B * H * W, 1), np.int64), np.tile(x.ravel(), B)[:, None], np.tile(y.ravel(), B)[:, None], lab], axis=1)
    st = _segment_sums(node, vals.astype(np.int64), node_capacity)
    out = np.zeros((node_capacity, 8), np.float32)
    has = st[:, 0] > 0
    a = st[has, 0]
    f64 = lambda v: v.astype(np.float64)  # noqa: E731
    out[has, 0] = (f64(st[has, 3]) / f64(400 * a)).astype(np.float32)
    out[has, 1] = (f64(st[has, 4]) / f64(512 * a)).astype(np.float32)
    out[has, 2] = (f64(st[has, 5]) / f64(512 * a)).astype(np.float32)
    out[has, 3] = (f64(2 * st[has, 1] + a) / f64(2 * a * W)).astype(np.float32)
    out[has, 4] = (f64(2 * st[has, 2] + a) / f64(2 * a * H)).astype(np.float32)
    out[has, 5] = (f64(a) / np.float64(H * W)).astype(np.float32)
    return out, st


def pool_quant(v):
    """float32 array -> int64 round_half_even(clamp(v, -65536, 65536) * 2^20), NaN -> 0 (the product is exact in float32)"""
    v = np.asarray(v, np.float32)
    c = np.clip(np.where(np.isnan(v), np.float32(0), v), np.float32(-65536), np.float32(65536)).astype(np.float32)
    return np.rint(c * np.float32(1048576.0)).astype(np.int64)


def pool(feat_nhwc, c_off, D, labels, offsets, node_capacity):
    """feat float32 (B, H, W, ld) -> float32 (node_capacity, D): (float)((double)sum q / (double)area * 2^-20), 0 without pixels"""
    feat = np.asarray(feat_nhwc, np.float32)
    node = _nodes(labels, offsets, node_capacity).ravel()
    q = pool_quant(feat[..., c_off:c_off + D]).reshape(-1, D)
    sums = _segment_sums(node, np.concatenate([q, np.ones((q.shape[0], 1), np.int64)], axis=1), node_capacity)
    area = sums[:, D]
    out = np.zeros((node_capacity, D), np.float32)
    has = area > 0
    out[has] = (sums[has, :D].astype(np.float64) / area[has, None].astype(np.float64) * 2.0 ** -20).astype(np.float32)
    return out


# ---- scenes shared by the host and the GPU tests ------------------------------------------------------------------------------------
def disc_scene(H=64, W=96, sigma=6.0, seed=3, discs=6):
    """background (40, 90, 35) with `discs` discs of (230, 170, 40), radius 6..13, and Gaussian pixel noise -> uint8 (H, W, 3)"""
    rng = np.random.default_rng(seed)
    img = np.empty((H, W, 3), np.float64)
    img[:] = (40, 90, 35)
    y, x = np.mgrid[0:H, 0:W]
    for _ in range(discs):
        cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(6, 13)
        img[(x - cx) ** 2 + (y - cy) ** 2 <= r * r] = (230, 170, 40)
    img += rng.normal(0.0, sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)
