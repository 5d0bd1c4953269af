"""Deterministic cases and the oracles for the border weight map (csrc/border.hip, include/mgunet.h "border weight map"), in plain
numpy on the CPU.  Imported by tests/test_border_host.py (the oracles against each other, the cases against wrong readings of the
definition: no GPU) and tests/test_gpu_border.py (the kernels).

Two oracles of (d1sq, d2sq, nearest): `brute` follows the definition (per label the minimum of the integer squared distances, the
pairs sorted by (distance, label)); `by_edt` takes scipy.ndimage.distance_transform_edt(return_indices=True) per label and recomputes
the squared distances in integers from the indices.  `weights` is the float64 weight, `separated` the target.  `method` is the
kernels' own two-pass method (two candidates per column, the row walk with its stopping rule) in vectorised numpy: it shows on the
CPU that the method is exact, and its switches are the wrong variants the cases must tell apart."""
from functools import lru_cache

import numpy as np

NONE = 1 << 30                     # MGU_D2_NONE
G_NONE = 1 << 15
VARIANTS = ("second_pixel", "one_per_column", "cityblock", "forget_older_run", "sum_of_squares", "tie_larger")
CW3 = (0.5, 2.0, 1.25)


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def _label_distances(lab, cityblock=False):
    """(labels ascending (L,), D (L, H, W) int64): D_k(p) of every object label of one image"""
    H, W = lab.shape
    ids = np.unique(lab[lab != 0])
    yy, xx = np.mgrid[0:H, 0:W]
    D = np.empty((len(ids), H, W), np.int64)
    for k, v in enumerate(ids):
        qy, qx = np.nonzero(lab == v)
        dy, dx = yy[..., None] - qy, xx[..., None] - qx
        D[k] = ((np.abs(dy) + np.abs(dx)) ** 2 if cityblock else dy * dy + dx * dx).min(-1)
    return ids.astype(np.int64), D


def _two_nearest(ids, D, shape, tie_larger=False):
    d1, d2 = np.full(shape, NONE, np.int64), np.full(shape, NONE, np.int64)
    near = np.zeros(shape, np.int64)
    if len(ids):
        if tie_larger:
            ids, D = ids[::-1], D[::-1]
        order = np.argsort(D, axis=0, kind="stable")          # equal distances keep the label order
        d1 = np.take_along_axis(D, order[:1], 0)[0]
        near = ids[order[0]]
        if len(ids) > 1:
            d2 = np.take_along_axis(D, order[1:2], 0)[0]
    return d1.astype(np.int32), d2.astype(np.int32), near.astype(np.int32)


def brute(labels, variant=None):
    """(d1sq, d2sq, nearest) int32 (B, H, W) by the definition; variant: one of the wrong readings this oracle can take"""
    out = []
    for lab in np.asarray(labels):
        ids, D = _label_distances(lab, cityblock=variant == "cityblock")
        d1, d2, near = _two_nearest(ids, D, lab.shape, tie_larger=variant == "tie_larger")
        if variant == "second_pixel" and (lab != 0).sum() > 1:   # the second-nearest labelled PIXEL, whatever its label
            qy, qx = np.nonzero(lab)
            yy, xx = np.mgrid[0:lab.shape[0], 0:lab.shape[1]]
            d2 = np.sort((yy[..., None] - qy) ** 2 + (xx[..., None] - qx) ** 2, axis=-1)[..., 1].astype(np.int32)
        out.append((d1, d2, near))
    return tuple(np.stack(v) for v in zip(*out))


def by_edt(labels):
    """the same from scipy's Euclidean feature transform per label, distances recomputed in integers from its indices"""
    from scipy.ndimage import distance_transform_edt
    out = []
    for lab in np.asarray(labels):
        H, W = lab.shape
        ids = np.unique(lab[lab != 0]).astype(np.int64)
        yy, xx = np.mgrid[0:H, 0:W]
        D = np.empty((len(ids), H, W), np.int64)
        for k, v in enumerate(ids):
            iy, ix = distance_transform_edt(lab != v, return_distances=False, return_indices=True)
            D[k] = (yy - iy).astype(np.int64) ** 2 + (xx - ix).astype(np.int64) ** 2
        out.append(_two_nearest(ids, D, lab.shape))
    return tuple(np.stack(v) for v in zip(*out))


def weights(d1sq, d2sq, classes, class_weight, w0, sigma, variant=None):
    """float64 (B, H, W): class_weight[cls] + w0 exp(-(sqrt d1sq + sqrt d2sq)^2 / (2 sigma^2)), the exponential term 0 where d2sq is NONE"""
    d1, d2 = np.asarray(d1sq, np.float64), np.asarray(d2sq, np.float64)
    s2 = d1 + d2 if variant == "sum_of_squares" else (np.sqrt(d1) + np.sqrt(d2)) ** 2
    e = np.where(np.asarray(d2sq) == NONE, 0.0, np.float64(w0) * np.exp(-s2 / (2.0 * np.float64(sigma) ** 2)))
    cw = np.ones(d1.shape, np.float64)
    if classes is not None and class_weight is not None:
        w = np.asarray(class_weight, np.float32).astype(np.float64)
        ok = (classes >= 0) & (classes < len(w))
        cw = np.where(ok, w[np.where(ok, classes, 0)], 0.0)
    return cw + e


def separated(labels, classes, background_class):
    """int64 (B, H, W): classes with every object pixel that has a 4-neighbour of another object set to background_class"""
    lab = np.asarray(labels)
    touch = np.zeros(lab.shape, bool)
    for axis, sl_a, sl_b in ((1, np.s_[:, 1:, :], np.s_[:, :-1, :]), (2, np.s_[:, :, 1:], np.s_[:, :, :-1])):
        a, b = lab[sl_a], lab[sl_b]
        diff = (a != 0) & (b != 0) & (a != b)
        touch[sl_a] |= diff
        touch[sl_b] |= diff
    return np.where(touch, np.int64(background_class), classes).astype(np.int64)


# ---- the kernels' method ----------------------------------------------------------------------------------------------------------------
def _before(d, l, d0, l0, tie_larger):
    return (d < d0) | ((d == d0) & ((l > l0) if tie_larger else (l < l0)))


def _merge(s, d, l, m, tie_larger=False):
    """bw_merge of csrc/border.hip on arrays: the entries (d, l) where m into the states s = [d1, l1, d2, l2]"""
    d1, l1, d2, l2 = s
    m = m & (d < NONE)
    e1 = m & (l == l1)
    d1 = np.where(e1 & (d < d1), d, d1)
    e2 = m & ~e1 & (l == l2)
    upd = e2 & (d < d2)
    d2n = np.where(upd, d, d2)
    sw = upd & _before(d2n, l2, d1, l1, tie_larger)
    d1, l1, d2, l2 = np.where(sw, d2n, d1), np.where(sw, l2, l1), np.where(sw, d1, d2n), np.where(sw, l1, l2)
    o = m & ~e1 & ~e2
    f = o & _before(d, l, d1, l1, tie_larger)
    g = o & ~f & _before(d, l, d2, l2, tie_larger)
    return [np.where(f, d, d1), np.where(f, l, l1), np.where(f, d1, np.where(g, d, d2)), np.where(f, l1, np.where(g, l, l2))]


def _column_scan(lab, ys, forget):
    """per pixel the last two runs of distinct labels met on the way along ys: (g1, a1, g2, a2), g the distance along the column"""
    H, W = lab.shape
    a1, y1, a2, y2 = (np.zeros(W, np.int64) for _ in range(4))
    out = np.zeros((4, H, W), np.int64)
    for y in ys:
        l = lab[y].astype(np.int64)
        nz = l != 0
        other = nz & (l != a1)
        back = other & (l == a2)                               # A, B, A: the variant drops B here
        a2, y2 = np.where(other, a1, a2), np.where(other, y1, y2)
        a1, y1 = np.where(other, l, a1), np.where(nz, y, y1)
        if forget:
            a2 = np.where(back, 0, a2)
        out[0, y], out[1, y] = np.where(a1 != 0, abs(y - y1), G_NONE), a1
        out[2, y], out[3, y] = np.where(a2 != 0, abs(y - y2), G_NONE), a2
    return out


def method(labels, variant=None):
    """(d1sq, d2sq, nearest) by the two passes of csrc/border.hip.  variant "one_per_column" keeps one candidate per column,
    "forget_older_run" loses the older run when a column reads A, B, A, "tie_larger" breaks ties to the larger label."""
    tl = variant == "tie_larger"
    out = []
    for lab in np.asarray(labels):
        H, W = lab.shape
        dn = _column_scan(lab, range(H), variant == "forget_older_run")
        up = _column_scan(lab, range(H - 1, -1, -1), variant == "forget_older_run")
        s = [dn[0], dn[1], dn[2], dn[3]]
        yes = np.ones((H, W), bool)
        s = _merge(s, up[0], up[1], yes & (up[1] != 0), tl)
        s = _merge(s, up[2], up[3], yes & (up[3] != 0), tl)
        c1, c2 = np.minimum(s[0] * s[0], NONE), np.minimum(s[2] * s[2], NONE)
        k1, k2 = s[1], s[3]
        if variant == "one_per_column":
            c2, k2 = np.full((H, W), NONE, np.int64), np.zeros((H, W), np.int64)
        b = [c1.copy(), k1.copy(), c2.copy(), k2.copy()]
        xs = np.arange(W)[None, :]
        for dx in range(1, W):
            dd = dx * dx
            walking = dd <= b[2]                               # the kernel's stopping rule: break when dx^2 > d2sq
            if not walking.any():
                break
            for sgn in (-1, 1):
                src = xs + sgn * dx
                ok = walking & (src >= 0) & (src < W)
                src = np.broadcast_to(np.clip(src, 0, W - 1), (H, W))
                rows = np.arange(H)[:, None]
                b = _merge(b, dd + c1[rows, src], k1[rows, src], ok & (c1[rows, src] < NONE), tl)
                b = _merge(b, dd + c2[rows, src], k2[rows, src], ok & (c2[rows, src] < NONE), tl)
        out.append((b[0].astype(np.int32), b[2].astype(np.int32), b[1].astype(np.int32)))
    return tuple(np.stack(v) for v in zip(*out))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def _blob(lab, y0, y1, x0, x1, v):
    lab[y0:y1, x0:x1] = v


def _random(seed, B, H, W, ids, density):
    r = np.random.RandomState(seed)
    pick = np.asarray(ids, np.int64)[r.randint(0, len(ids), (B, H, W))]
    return np.where(r.random_sample((B, H, W)) < density, pick, 0).astype(np.int32)


def _classes_of(lab, ncls=3):
    """a class map that follows the objects: class 1 + (|label| % (ncls - 1)) on them, 0 on background"""
    l = lab.astype(np.int64)
    return np.where(l != 0, 1 + np.abs(l) % (ncls - 1), 0).astype(np.int64)


@lru_cache(maxsize=None)
def cases():
    """name -> dict(labels int32 (B, H, W), classes int64 (B, H, W) or None, class_weight or None, w0, sigma, background)"""
    out = {}

    def add(name, lab, classes="follow", class_weight=CW3, w0=10.0, sigma=5.0, background=0):
        lab = np.ascontiguousarray(lab, dtype=np.int32)
        if lab.ndim == 2:
            lab = lab[None]
        cl = _classes_of(lab) if isinstance(classes, str) else classes
        out[name] = {"labels": lab, "classes": cl, "class_weight": class_weight, "w0": w0, "sigma": sigma, "background": background}

    add("1x1_empty", np.zeros((1, 1)))
    add("1x1_object", np.full((1, 1), 5))
    row = np.zeros((1, 70))
    row[0, [3, 4, 20, 41, 69]] = [2, 2, 9, 4, 2]
    add("1xW", row)
    add("Hx1", row.T[:64])
    for W in (63, 64, 65, 255, 257, 300):                      # the lane stride of the column pass, the workgroup stride of the row pass
        add(f"w{W}", _random(W, 2, 5, W, (1, 2, 3, 4, 5, 6), 0.04), sigma=3.0)
    add("none", np.zeros((2, 6, 9)))
    one = np.zeros((7, 11))
    _blob(one, 2, 4, 3, 6, 4)
    add("one", one)
    two = one.copy()
    _blob(two, 5, 7, 8, 11, 1)
    add("two", two, sigma=2.0)
    mixed = np.zeros((3, 9, 12))                               # images of one batch never mix: 0, 1 and 3 objects, label 7 in two of them
    _blob(mixed[1], 1, 3, 1, 3, 7)
    _blob(mixed[2], 6, 9, 9, 12, 7)
    _blob(mixed[2], 0, 2, 0, 2, 3)
    _blob(mixed[2], 4, 5, 4, 6, 11)
    add("mixed_batch", mixed, sigma=4.0)
    abaa = np.zeros((9, 5))                                     # a column reading A, B, A, A: the two-run stack
    abaa[:4, 2] = [6, 8, 6, 6]
    add("abaa_column", abaa)
    add("abaa_alone", np.array([[6], [8], [6], [6], [0], [0], [0]]))
    add("tie_row", np.array([[7, 0, 0, 0, 3]]))                 # the middle pixel: d1sq == d2sq == 4, nearest 3
    late = np.zeros((5, 5))                                     # (2, 2): 5 above and 7 below at distance 2 give d1sq == d2sq == 4 from
    late[0, 2], late[4, 2], late[2, 0] = 5, 7, 1                # its own column; label 1 at dx = 2 (dx^2 == d2sq) still wins `nearest`
    add("tie_late_smaller_label", late)
    ids = np.zeros((6, 40))
    ids[1, 2], ids[4, 9], ids[2, 20], ids[5, 33], ids[0, 39] = -5, 2 ** 31 - 1, -2 ** 31, 1000000, -1
    add("negative_sparse_ids", ids, sigma=8.0)
    pieces = np.zeros((8, 30))
    _blob(pieces, 0, 2, 0, 3, 4)
    _blob(pieces, 6, 8, 26, 30, 4)                              # label 4 again, far away
    _blob(pieces, 3, 5, 12, 15, 9)
    add("disconnected", pieces)
    touch = np.zeros((2, 8, 10))
    _blob(touch[0], 1, 6, 1, 5, 1)
    _blob(touch[0], 1, 6, 5, 9, 2)                              # side by side
    _blob(touch[1], 0, 4, 2, 8, 3)
    _blob(touch[1], 4, 8, 2, 8, 1)                              # one above the other
    touch[1, 7, 9] = 5                                          # diagonal to nothing: stays
    add("touching", touch, background=0)
    add("touching_background_2", touch, background=2)
    corner = np.zeros((64, 700))
    corner[63, 699] = 3
    add("far_corner", corner)                                   # every pixel walks its whole row
    H, W = 9, 13
    yy, xx = np.mgrid[0:H, 0:W]
    add("checkerboard", np.where((yy + xx) % 2 == 0, 1 + yy * W + xx, 0), sigma=1.0)
    ign = _random(5, 2, 11, 17, (1, 2, 3), 0.08)
    cl = _classes_of(ign)
    cl[:, :3] = -100
    cl[1, 5, 5] = 7                                             # outside the weights too
    add("class_ignore", ign, classes=cl)
    add("no_classes", ign, classes=None, class_weight=None)
    add("classes_no_weights", ign, classes=cl, class_weight=None)
    add("w0_zero", ign, w0=0.0)
    add("random_sparse", _random(11, 3, 23, 37, (1, 2, 3, 4, 5, 6, 7, 8, 9), 0.02))
    add("random_dense", _random(12, 3, 23, 37, (-3, 1, 2, 50), 0.5), sigma=1.5)
    add("random_two_labels", _random(13, 2, 31, 70, (4, 9), 0.01), sigma=12.0)
    return out


@lru_cache(maxsize=None)
def expected(name):
    """the oracle's outputs of a case, computed once: dict(d1sq, d2sq, nearest, weight float64, target or None)"""
    c = cases()[name]
    d1, d2, near = brute(c["labels"])
    w = weights(d1, d2, c["classes"], c["class_weight"], c["w0"], c["sigma"])
    tgt = None if c["classes"] is None else separated(c["labels"], c["classes"], c["background"])
    for a in (d1, d2, near, w):
        a.setflags(write=False)
    return {"d1sq": d1, "d2sq": d2, "nearest": near, "weight": w, "target": tgt}
