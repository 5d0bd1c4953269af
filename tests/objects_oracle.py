"""numpy oracle of mgunet.connected_components, shared by the object tests: skimage.measure.label semantics (pixels join when they
are neighbours holding the same foreground value) and numbering (raster order of each object's first pixel), plus the per-object
statistics.  Vectorised hook-and-jump union-find, fast enough for 1024 x 1024 maps on the host."""
import numpy as np

OFFSETS = {1: ((0, -1), (-1, 0)), 2: ((0, -1), (-1, 0), (-1, -1), (-1, 1))}


def foreground(m, background=0, num_classes=None):
    fg = m != background
    if num_classes is not None:
        fg &= (m >= 0) & (m < num_classes)
    return fg


def label(m, connectivity=2, background=0, num_classes=None, min_area=0):
    """int32 labels of one (H, W) map."""
    m = np.asarray(m)
    H, W = m.shape
    fg = foreground(m, background, num_classes)
    idx = np.arange(H * W).reshape(H, W)
    us, vs = [], []
    for dy, dx in OFFSETS[connectivity]:
        y0, x0, x1 = max(0, -dy), max(0, -dx), W - max(0, dx)
        a, b = (slice(y0, H), slice(x0, x1)), (slice(y0 + dy, H + dy), slice(x0 + dx, x1 + dx))
        join = fg[a] & fg[b] & (m[a] == m[b])
        us.append(idx[a][join])
        vs.append(idx[b][join])
    u, v = np.concatenate(us), np.concatenate(vs)
    par = np.where(fg.reshape(-1), np.arange(H * W), -1)
    while True:
        while True:   # pointer jumping: every foreground pixel at its root
            nxt = np.where(par >= 0, par[np.maximum(par, 0)], -1)
            if np.array_equal(nxt, par):
                break
            par = nxt
        ru, rv = par[u], par[v]
        diff = ru != rv
        if not diff.any():
            break
        hi, lo = np.maximum(ru[diff], rv[diff]), np.minimum(ru[diff], rv[diff])
        np.minimum.at(par, hi, lo)   # hook larger roots under smaller ones: a root is its component's smallest index
    flat = np.arange(H * W)
    roots = par == flat
    if min_area:
        area = np.bincount(par[par >= 0], minlength=H * W)
        roots &= area >= min_area
    num = np.cumsum(roots)
    out = np.where(par >= 0, np.where(roots[np.maximum(par, 0)], num[np.maximum(par, 0)], 0), 0)
    return out.reshape(H, W).astype(np.int32)


def stats(labels, values):
    """class, area, bbox [xmin, ymin, xmax, ymax) and [sum x, sum y] of objects 1..n of one labelled map, in label order."""
    n = int(labels.max()) if labels.size else 0
    ys, xs = np.nonzero(labels)
    lab = labels[ys, xs].astype(np.int64) - 1
    area = np.bincount(lab, minlength=n)
    sx, sy = np.bincount(lab, xs, minlength=n).astype(np.int64), np.bincount(lab, ys, minlength=n).astype(np.int64)
    bbox = np.zeros((n, 4), np.int64)
    cls = np.zeros(n, np.int64)
    if n:
        bbox[:, 0] = np.full(n, np.iinfo(np.int64).max)
        bbox[:, 1] = np.full(n, np.iinfo(np.int64).max)
        np.minimum.at(bbox[:, 0], lab, xs)
        np.minimum.at(bbox[:, 1], lab, ys)
        np.maximum.at(bbox[:, 2], lab, xs + 1)
        np.maximum.at(bbox[:, 3], lab, ys + 1)
        cls[lab] = np.asarray(values)[ys, xs]
    return cls, area.astype(np.int64), bbox, np.stack([sx, sy], 1)
