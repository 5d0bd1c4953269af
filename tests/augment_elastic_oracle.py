"""numpy restatement of mgu_augment_elastic_color and mgu_elastic_field (include/mgunet.h, "elastic deformation"): int64 throughout,
vectorised over the output pixels of one image.  It takes the integer parameter table and the integer control nodes, so equality with
the device does not depend on anyone's libm.  The colour step, the normalisation and the luma sums are augment_affine_oracle's; the
sampling is restated here on explicit coordinates (the host test shows it equal to augment_affine_oracle's with zero control).
`variant` names one wrong reading of the definition (VARIANTS); the host test shows that the shared cases tell each of them from the
definition."""
import numpy as np

import augment_affine_oracle as AO

VARIANTS = ("su_rounded", "no_half_pixel", "t_rounded", "weights_unnormalised", "remainder_to_w1_always", "round_between_passes",
            "planes_swapped", "nodes_transposed", "field_no_round", "shift_toward_zero", "int32_wrap", "catmull_rom", "labels_floor")
T = 256
CTRL_LIMIT = 1 << 26


def _shr(v, n, variant):
    if variant == "shift_toward_zero":
        return np.where(v >= 0, v >> n, -((-v) >> n))
    return v >> n


def weights_q14(variant=None) -> np.ndarray:
    """Wq (256, 4) int64 from Python integers"""
    rows = []
    for t in range(T):
        if variant == "catmull_rom":
            D = 2 * T ** 3
            n = (-t ** 3 + 2 * T * t * t - T * T * t, 3 * t ** 3 - 5 * T * t * t + 2 * T ** 3, -3 * t ** 3 + 4 * T * t * t + T * T * t, t ** 3 - T * t * t)
        else:
            D = 6 * T ** 3
            n = ((T - t) ** 3, 3 * t ** 3 - 6 * T * t * t + 4 * T ** 3, -3 * t ** 3 + 3 * T * t * t + 3 * T * T * t + T ** 3, t ** 3)
        assert sum(n) == D
        w = [(2 * 16384 * v + D) // (2 * D) for v in n]
        rem = 16384 - sum(w)
        if variant == "weights_unnormalised":
            pass
        elif variant == "remainder_to_w1_always":
            w[1] += rem
        else:
            w[2 if w[2] > w[1] else 1] += rem
        rows.append(w)
    return np.asarray(rows, np.int64)


def lattice(g: int, size: int, variant=None):
    """(cell index, fraction index) int64 (size,) of the pixels 0..size-1 along one axis with g nodes"""
    if variant == "su_rounded":
        su = (2 * ((g - 3) << 16) + size) // (2 * size)
    else:
        su = ((g - 3) << 16) // size
    u = np.arange(size, dtype=np.int64) * su + (0 if variant == "no_half_pixel" else su >> 1)
    if variant == "t_rounded":
        u = u + 128
    i = u >> 16
    if variant is None:
        assert i.min() >= 0 and i.max() <= g - 4
    return np.clip(i, 0, g - 4), (u >> 8) & 255       # the clip only keeps a wrong variant inside the arrays


def field(ctrl, out_hw, variant=None):
    """ctrl (2, gh, gw) ints -> (Dx, Dy) int64 (H, W)"""
    c = np.asarray(ctrl).astype(np.int64)
    _two, gh, gw = c.shape
    if variant is None:
        assert 4 <= gh <= 32 and 4 <= gw <= 32 and np.abs(c).max() <= CTRL_LIMIT
    if variant == "planes_swapped":
        c = c[::-1]
    if variant == "nodes_transposed":
        c = c.reshape(2, gw, gh).transpose(0, 2, 1)
    H, W = int(out_hw[0]), int(out_hw[1])
    Wq = weights_q14(variant)
    j, s = lattice(gh, H, variant)
    i, t = lattice(gw, W, variant)
    out = []
    for pl in range(2):
        q = sum(Wq[s, b][:, None] * c[pl][j + b, :] for b in range(4))                  # (H, gw): the row's column sums
        if variant == "round_between_passes":
            q = (q + (1 << 13)) >> 14
        if variant == "int32_wrap":
            q = ((q + 2 ** 31) % 2 ** 32) - 2 ** 31
        acc = sum(Wq[t, a][None, :] * q[:, i + a] for a in range(4))                    # (H, W)
        if variant == "round_between_passes":
            out.append((acc + (1 << 13)) >> 14)
        elif variant == "field_no_round":
            out.append(acc >> 28)
        else:
            out.append(_shr(acc + (1 << 27), 28, variant))
    return out[0], out[1]


def field_direct(ctrl, out_hw):
    """the field as the definition writes it: the double sum over the sixteen nodes, per pixel, in Python integers"""
    c = np.asarray(ctrl).astype(np.int64).tolist()
    gh, gw = len(c[0]), len(c[0][0])
    H, W = int(out_hw[0]), int(out_hw[1])
    Wq = weights_q14().tolist()
    su, sv = ((gw - 3) << 16) // W, ((gh - 3) << 16) // H
    out = np.zeros((2, H, W), np.int64)
    for y in range(H):
        v = y * sv + (sv >> 1)
        j, s = v >> 16, (v >> 8) & 255
        for x in range(W):
            u = x * su + (su >> 1)
            i, t = u >> 16, (u >> 8) & 255
            for pl in range(2):
                acc = sum(Wq[s][b] * Wq[t][a] * c[pl][j + b][i + a] for b in range(4) for a in range(4))
                out[pl, y, x] = (acc + (1 << 27)) >> 28
    return out[0], out[1]


def coordinates(row, ctrl, out_hw, variant=None):
    """(sx, sy) int64 (H, W); ctrl None: the affine coordinates"""
    sx, sy = AO.coordinates(row, out_hw)
    if ctrl is not None:
        dx, dy = field(ctrl, out_hw, variant)
        sx, sy = sx + dx, sy + dy
    return sx, sy


def sample_image_at(img_rgb, sx, sy, fill=(0, 0, 0), variant=None):
    """the bilinear bytes (H, W, 3) int64 at the 16.16 coordinates, before the colour step"""
    Hs, Ws = img_rgb.shape[:2]
    src = img_rgb.astype(np.int64)
    ix, iy = _shr(sx, 16, variant), _shr(sy, 16, variant)
    fx, fy = _shr(sx, 8, variant) & 255, _shr(sy, 8, variant) & 255
    fillv = np.asarray(fill, np.int64)

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
        return np.where(inside[..., None], src[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)], fillv)

    acc = ((256 - fx) * (256 - fy))[..., None] * tap(ix, iy) + (fx * (256 - fy))[..., None] * tap(ix + 1, iy) \
        + ((256 - fx) * fy)[..., None] * tap(ix, iy + 1) + (fx * fy)[..., None] * tap(ix + 1, iy + 1)
    return (acc + 32768) >> 16


def sample_nearest_at(m, sx, sy, fill, num_classes=0, half=32768, variant=None):
    """nearest sample of an (Hs, Ws) integer map -> int64 (H, W); num_classes > 0 clips the values inside the source"""
    Hs, Ws = m.shape
    mx, my = _shr(sx + half, 16, variant), _shr(sy + half, 16, variant)
    inside = (mx >= 0) & (mx < Ws) & (my >= 0) & (my < Hs)
    v = m.astype(np.int64)[np.clip(my, 0, Hs - 1), np.clip(mx, 0, Ws - 1)]
    if num_classes > 0:
        v = np.clip(v, 0, num_classes - 1)
    return np.where(inside, v, np.int64(fill))


def interior(img_hw, sx, sy):
    """bool (H, W): all four taps of the pixel lie inside the source"""
    ix, iy = sx >> 16, sy >> 16
    return (ix >= 0) & (ix + 1 < img_hw[1]) & (iy >= 0) & (iy + 1 < img_hw[0])


def control(normals, sigma, row):
    """elastic_control in Python integers -> (cx, cy) nested lists (gh, gw)"""
    n = np.asarray(normals, np.float64)
    a0, a1, _a2, a3, a4 = (int(v) for v in row[:5])

    def fix16(v):
        return int(np.floor(float(sigma) * min(max(float(v), -3.0), 3.0) * 65536.0 + 0.5))

    cx = [[(a0 * fix16(x) + a1 * fix16(y) + 32768) >> 16 for x, y in zip(rx, ry)] for rx, ry in zip(n[0].tolist(), n[1].tolist())]
    cy = [[(a3 * fix16(x) + a4 * fix16(y) + 32768) >> 16 for x, y in zip(rx, ry)] for rx, ry in zip(n[0].tolist(), n[1].tolist())]
    return cx, cy


def augment(images_u8, table, ctrl, out_hw, mean, std, masks=None, labels=None, fill=(0, 0, 0), mask_fill=-100, label_fill=0, num_classes=0,
            bgr=False, variant=None):
    """images_u8 (B, Hs, Ws, 3) uint8, table (B, 16) ints, ctrl (B, 2, gh, gw) ints or None, masks optional (B, Hs, Ws) uint8, labels
    optional (B, Hs, Ws) int32 -> (out float32 (B, 3, H, W), bytes uint8 (B, H, W, 3) after the colour step, masks int64 (B, H, W) | None,
    labels int32 (B, H, W) | None)"""
    images_u8, table = np.asarray(images_u8), np.asarray(table).astype(np.int64)
    B, Hs, Ws, _ = images_u8.shape
    outs, byts, ms, ls = [], [], [], []
    for b in range(B):
        rgb = images_u8[b][..., ::-1] if bgr else images_u8[b]
        row = table[b].tolist()
        sx, sy = coordinates(row, None if ctrl is None else np.asarray(ctrl)[b], out_hw, variant)
        v = sample_image_at(rgb, sx, sy, fill, variant)
        q = AO.colour(v, row, AO.mean_q8(AO.luma_sum(rgb), Hs * Ws), variant if variant == "shift_toward_zero" else None)
        byts.append(q.astype(np.uint8)), outs.append(AO.normalize(q, mean, std))
        if masks is not None:
            ms.append(sample_nearest_at(np.asarray(masks)[b], sx, sy, mask_fill, num_classes, variant=variant))
        if labels is not None:
            ls.append(sample_nearest_at(np.asarray(labels)[b], sx, sy, label_fill, 0, 0 if variant == "labels_floor" else 32768,
                                        variant).astype(np.int32))
    return np.stack(outs), np.stack(byts), (np.stack(ms) if masks is not None else None), (np.stack(ls) if labels is not None else None)
