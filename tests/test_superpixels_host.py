"""CPU tests that pin tests/superpixels_oracle.py -- the numpy definition the GPU tests of the superpixel-graph stages compare with bit
for bit -- against float64 CIELAB, per-pixel brute-force loops, scipy.ndimage.label and hand-made cases.  No GPU, no library call."""
import numpy as np
import pytest
from scipy import ndimage

import mgunet
import superpixels_oracle as SO


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def lab_f64(rgb):
    v = rgb.astype(np.float64) / 255.0
    lin = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    m = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]])
    xyz = lin @ (m / m.sum(1, keepdims=True)).T
    d = 6.0 / 29.0
    f = np.where(xyz > d ** 3, np.cbrt(xyz), xyz / (3 * d * d) + 4.0 / 29.0)
    return np.stack([116 * f[..., 1] - 16, 500 * (f[..., 0] - f[..., 1]), 200 * (f[..., 1] - f[..., 2])], -1)


def test_tables_rows_ranges_and_distance_from_float64_lab():
    LIN, M, F = mgunet.lab_tables()
    assert LIN.dtype == np.uint16 and M.dtype == np.int32 and F.dtype == np.uint16
    assert M.tolist() == [[1777, 1541, 778], [871, 2929, 296], [73, 448, 3575]] and M.sum(1).tolist() == [4096] * 3
    assert (int(LIN[0]), int(LIN[255]), int(F.min()), int(F.max())) == (0, 4095, 141, 1024)
    g = np.arange(0, 256, 3, dtype=np.uint8)
    rgb = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    q = SO.rgb_to_lab_q(rgb)
    assert [(int(q[:, k].min()), int(q[:, k].max())) for k in range(3)] == [(0, 400), (-346, 393), (-431, 378)]
    err = np.abs(q / 4.0 - lab_f64(rgb)).max(0)
    print("largest deviation from float64 Lab (L, a, b):", err)
    assert err[0] <= 0.5 and err[1] <= 1.5 and err[2] <= 0.75


# ---- assignment and update ------------------------------------------------------------------------------------------------------------
def brute_slic(rgb, S, mq, T):
    """per-pixel Python loops, Python integers"""
    H, W = rgb.shape[:2]
    lab = SO.rgb_to_lab_q(rgb).tolist()
    gx, gy = -(-W // S), -(-H // S)
    cen = []
    for i in range(gy):
        for j in range(gx):
            x, y = min(j * S + S // 2, W - 1), min(i * S + S // 2, H - 1)
            cen.append([x, y] + lab[y][x] + [0])
    for t in range(T):
        labels = [[0] * W for _ in range(H)]
        for y in range(H):
            for x in range(W):
                best, bk = None, -1
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        ii, jj = y // S + di, x // S + dj
                        if not (0 <= ii < gy and 0 <= jj < gx):
                            continue
                        c = cen[ii * gx + jj]
                        D = sum((lab[y][x][q] - c[2 + q]) ** 2 for q in range(3)) * S * S + mq * mq * ((x - c[0]) ** 2 + (y - c[1]) ** 2)
                        if best is None or D < best:
                            best, bk = D, ii * gx + jj
                labels[y][x] = bk
        if t + 1 < T:
            for k in range(gx * gy):
                px = [(x, y) for y in range(H) for x in range(W) if labels[y][x] == k]
                n = len(px)
                if n:
                    sums = [sum(p[0] for p in px), sum(p[1] for p in px)] + [sum(lab[y][x][q] for x, y in px) for q in range(3)]
                    cen[k][:5] = [(2 * s + n) // (2 * n) for s in sums]
                cen[k][5] = n
    return np.array(labels), np.array(cen)


@pytest.mark.parametrize("H,W,S,T", [(1, 1, 4, 1), (7, 5, 4, 3), (12, 12, 4, 4), (9, 12, 5, 2)])
def test_vectorised_slic_equals_the_per_pixel_loop(H, W, S, T):
    rng = np.random.default_rng(H * 100 + W)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgb[:, W // 2:] //= 3
    for mq in (4, 40):
        lb, cen = SO.slic(rgb[None], S, mq, T)
        rl, rc = brute_slic(rgb, S, mq, T)
        assert np.array_equal(lb[0], rl) and np.array_equal(cen[0], rc)


def test_uniform_image_gives_the_grid_voronoi_cells_with_ties_to_the_lower_index():
    """centres at x, y in {2, 6}: column 4 and row 4 are equally far from both, and go to the lower index"""
    rgb = np.full((1, 8, 8, 3), 77, np.uint8)
    top, bottom = [0, 0, 0, 0, 0, 1, 1, 1], [2, 2, 2, 2, 2, 3, 3, 3]
    want = np.array([top] * 5 + [bottom] * 3)
    assert np.array_equal(SO.slic(rgb, 4, 40, 1)[0][0], want)       # ties to the higher index would put column 4 and row 4 the other way


@pytest.mark.parametrize("colour", [(20, 230, 30), (25, 20, 235)])
def test_negative_sums_use_floor_division(colour):
    rng = np.random.default_rng(1)
    rgb = np.clip(np.array(colour) + rng.integers(-20, 21, (1, 12, 16, 3)), 0, 255).astype(np.uint8)
    lab = SO.rgb_to_lab_q(rgb[0])
    assert (lab[..., 1].sum() < 0) or (lab[..., 2].sum() < 0)
    cen0 = SO.slic_init_centres(lab, 4)
    lb = SO.slic_assign(lab, cen0, 4, 40)
    cen = SO.slic_update(lab, lb, cen0)
    saw_inexact_negative = False
    for k in range(cen.shape[0]):
        ys, xs = np.nonzero(lb == k)
        n = len(ys)
        if n == 0:
            assert np.array_equal(cen[k, :5], cen0[k, :5]) and cen[k, 5] == 0
            continue
        sums = [int(xs.sum()), int(ys.sum())] + [int(lab[ys, xs, q].sum()) for q in range(3)]
        assert cen[k].tolist() == [(2 * s + n) // (2 * n) for s in sums] + [n]
        saw_inexact_negative |= any(s < 0 and (2 * s + n) % (2 * n) for s in sums)
    assert saw_inexact_negative   # truncation would differ from floor somewhere


# ---- connect --------------------------------------------------------------------------------------------------------------------------
FOUR = ndimage.generate_binary_structure(2, 1)


def assert_partition_of_connected_regions(L, n):
    assert L.min() == 0 and L.max() == n - 1 and len(np.unique(L)) == n
    firsts = [np.flatnonzero(L.ravel() == k)[0] for k in range(n)]
    assert firsts == sorted(firsts)
    for k in range(n):
        assert ndimage.label(L == k, FOUR)[1] == 1, k


def test_components_equal_scipy_label_per_value():
    rng = np.random.default_rng(2)
    raw = rng.integers(0, 4, (2, 23, 31))
    labels, counts, offsets = SO.connect(raw, 0, 0)
    for b in range(2):
        total = 0
        for v in range(4):
            ref, m = ndimage.label(raw[b] == v, FOUR)
            total += m
            for r in range(1, m + 1):
                assert len(np.unique(labels[b][ref == r])) == 1
        assert counts[b] == total == len(np.unique(labels[b]))
        assert_partition_of_connected_regions(labels[b], int(counts[b]))
    assert offsets.tolist() == [0, int(counts[0]), int(counts.sum())]


def scene_history(rounds=2):
    raw, _ = SO.slic(SO.disc_scene()[None], 8, 40, 6)
    hist = []
    out = SO.connect(raw, 16, rounds, history=hist)
    return raw, out, hist[0]


def test_noise_scene_needs_two_merge_rounds():
    raw, (labels, counts, offsets), steps = scene_history()
    (L0, n0, _), (L1, n1, m1), (L2, n2, m2) = steps
    small1 = int((np.bincount(L1.ravel()) < 16).sum())
    print(f"components {n0}; after round 1: {n1} regions, {small1} small; after round 2: {n2} regions, "
          f"{int((np.bincount(L2.ravel()) < 16).sum())} small")
    assert m1 >= 1 and n1 == n0 - m1
    assert small1 >= 1
    assert m2 >= 1 and n2 == n1 - m2
    for L, n, _ in steps:
        assert_partition_of_connected_regions(L, n)
    assert np.array_equal(labels[0], L2) and counts[0] == n2


def test_checkerboard_of_single_pixels_never_merges():
    raw = (np.indices((6, 9)).sum(0) % 2)[None]
    labels, counts, _ = SO.connect(raw, 4, 3)
    assert counts[0] == 54 and np.array_equal(labels[0], np.arange(54).reshape(6, 9))


def test_merge_takes_the_longest_border_and_ties_go_to_the_earlier_region():
    raw = np.zeros((1, 6, 9), np.int64)
    raw[0, :, 5:] = 1
    raw[0, 2:4, 4] = 2                         # a 2-pixel region: 3 edges with region 0, 2 with region 1
    assert np.array_equal(SO.connect(raw, 3, 1)[0][0], (raw[0] == 1).astype(int))
    raw[0, 2:4, 4] = 0
    raw[0, 0, 4:6] = 2                         # 2 pixels on top: 2 edges with each side -> the earlier region (0)
    assert np.array_equal(SO.connect(raw, 3, 1)[0][0], (raw[0] == 1).astype(int))


# ---- adjacency ------------------------------------------------------------------------------------------------------------------------
def brute_adjacency(labels, offsets, cap):
    pairs = {}
    for b in range(labels.shape[0]):
        o0, n = int(offsets[b]), int(offsets[b + 1] - offsets[b])
        if offsets[b + 1] > cap:
            continue
        H, W = labels[b].shape
        for y in range(H):
            for x in range(W):
                for yy, xx in ((y, x + 1), (y + 1, x)):
                    if yy < H and xx < W:
                        p, q = int(labels[b, y, x]), int(labels[b, yy, xx])
                        if p != q and 0 <= p < n and 0 <= q < n:
                            pairs[(o0 + p, o0 + q)] = pairs.get((o0 + p, o0 + q), 0) + 1
                            pairs[(o0 + q, o0 + p)] = pairs.get((o0 + q, o0 + p), 0) + 1
    return pairs


def test_adjacency_equals_the_double_loop_and_is_planar_for_connected_regions():
    _, (labels, counts, offsets), _ = scene_history()
    both = np.concatenate([labels[:, :32, :40], labels[:, 20:52, 30:70]])
    lab2, cnt2, off2 = SO.connect(both, 0, 0)
    cap = int(off2[-1])
    rowptr, col, border, status = SO.adjacency(lab2, off2, cap)
    ref = brute_adjacency(lab2, off2, cap)
    got = {(r, int(col[e])): int(border[e]) for r in range(cap) for e in range(rowptr[r], rowptr[r + 1])}
    assert status == 0 and got == ref and rowptr[-1] == len(ref) == col.size
    for r in range(cap):
        row = col[rowptr[r]:rowptr[r + 1]]
        assert np.all(np.diff(row) > 0) and r not in row
    assert all(got[(v, u)] == w for (u, v), w in got.items())
    for b in range(2):
        N = int(cnt2[b])
        assert rowptr[off2[b + 1]] - rowptr[off2[b]] <= 6 * N - 12
    # labels outside [0, n_b) take no part; an image past the capacity contributes nothing and raises bit 2
    holes = lab2.copy()
    holes[0][holes[0] == 3] = -1
    rp, cl, _, _ = SO.adjacency(holes, off2, cap)
    assert rp[4] - rp[3] == 0 and 3 not in cl[: rp[off2[1]]]
    rp, cl, _, st = SO.adjacency(lab2, off2, cap - 1)
    assert st == 2 and rp[-1] == rp[off2[1]] and rp.size == cap


# ---- features and pool ----------------------------------------------------------------------------------------------------------------
def test_features_are_the_stated_expressions():
    img = SO.disc_scene(24, 40, seed=5)[None]
    raw, _ = SO.slic(img, 8, 40, 3)
    labels, counts, offsets = SO.connect(raw, 8, 1)
    cap = int(counts[0]) + 2
    feat, st = SO.features(img, labels, offsets, cap)
    lab = SO.rgb_to_lab_q(img[0])
    for k in range(int(counts[0])):
        ys, xs = np.nonzero(labels[0] == k)
        a = len(ys)
        sL, sa, sb = (int(lab[ys, xs, q].sum()) for q in range(3))
        assert st[k].tolist() == [a, int(xs.sum()), int(ys.sum()), sL, sa, sb]
        want = [sL / (400 * a), sa / (512 * a), sb / (512 * a), (2 * int(xs.sum()) + a) / (2 * a * 40), (2 * int(ys.sum()) + a) / (2 * a * 24),
                a / (24 * 40), 0.0, 0.0]
        assert np.array_equal(feat[k], np.array(want, np.float64).astype(np.float32))
    assert not feat[int(counts[0]):].any() and feat.dtype == np.float32


def test_pool_quantisation_and_its_bound_against_float64():
    assert SO.pool_quant(np.array([np.nan, 1e9, -1e9, 65536.0, 2.0 ** -21, 3 * 2.0 ** -21, 1.0], np.float32)).tolist() == \
        [0, 2 ** 36, -2 ** 36, 2 ** 36, 0, 2, 2 ** 20]
    rng = np.random.default_rng(7)
    labels = rng.integers(0, 5, (2, 9, 11)).astype(np.int32)
    offsets = np.array([0, 5, 10])
    feat = (rng.standard_normal((2, 9, 11, 7)) * np.array([1e-3, 1, 1, 50, 1, 1, 1])).astype(np.float32)
    got = SO.pool(feat, 1, 4, labels, offsets, 12)
    for b in range(2):
        for k in range(5):
            vals = feat[b][labels[b] == k][:, 1:5].astype(np.float64)
            mean = vals.mean(0)
            assert np.all(np.abs(got[5 * b + k] - mean) <= 2.0 ** -21 + 2.0 ** -24 * np.abs(mean))
    assert not got[10:].any()
