"""numpy form of the contrast-limited adaptive histogram equalisation the device computes (include/mgunet.h, mgu_clahe_u8), written from
the definition and sharing no code with the package.  Integers up to the table, float32 arrays after it: every float operation is a
numpy operation on float32 arrays, so each is rounded on its own.

    geometry    H % gy == 0 and W % gx == 0: He, We = H, W; else BOTH He = H + gy - H % gy, We = W + gx - W % gx (OpenCV's rule);
                th, tw = He / gy, We / gx; extended pixel (y, x) reads v[r(y, H)][r(x, W)], r = reflect-101 repeated until inside
    plane       1 channel: the image; 3 channels: Y of cv2's fixed-point RGB2YUV, the result cv2's YUV2RGB of (out, U, V)
    table       histogram of the tile's th * tw extended pixels; clip_limit > 0: cl = max(1, int(clip_limit * area / 256)), the excess
                over cl spread as excess / 256 to every bin and one more to the bins k * max(256 / residual, 1), k < residual;
                lut[i] = sat8(rint(float32(cumsum_i) * (float32(255) / float32(area))))
    pixel       txf = float32(x) * (1 / float32(tw)) - 0.5; tx1 = floor(txf); xa = txf - tx1; tx2 = min(tx1 + 1, gx - 1); tx1 = max(tx1, 0)
                (likewise y); out = sat8(rint((l11 xa1 + l12 xa) ya1 + (l21 xa1 + l22 xa) ya)), xa1 = 1 - xa

It follows OpenCV 4.x's clahe.cpp for 8-bit images; it has not been compared with a cv2 build."""
import numpy as np

F = np.float32


def geometry(H, W, gy, gx):
    """-> (He, We, th, tw)"""
    if H % gy == 0 and W % gx == 0:
        He, We = H, W
    else:
        He, We = H + gy - H % gy, W + gx - W % gx
    return He, We, He // gy, We // gx


def reflect(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def descale(v):
    return (v + (1 << 13)) >> 14


def rgb2yuv(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    Y = descale(r * 4899 + g * 9617 + b * 1868)
    U = np.clip(descale((b - Y) * 8061 + (128 << 14)), 0, 255)
    V = np.clip(descale((r - Y) * 14369 + (128 << 14)), 0, 255)
    return Y, U, V


def yuv2rgb(Y, U, V):
    u, v = U - 128, V - 128
    out = np.stack([Y + descale(v * 18678), Y + descale(u * -6472 + v * -9519), Y + descale(u * 33292)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def clip_value(clip_limit, area):
    """the integer limit of a bin; 0: no clipping"""
    if not clip_limit > 0:
        return 0
    return max(1, int(float(clip_limit) * area / 256))


def histograms(v, gy, gx):
    """v: (B, H, W) integers in 0..255 -> (B, gy, gx, 256) int64 counts over the extended tiles"""
    B, H, W = v.shape
    He, We, th, tw = geometry(H, W, gy, gx)
    ry = np.array([reflect(i, H) for i in range(He)], np.int64)
    rx = np.array([reflect(i, W) for i in range(We)], np.int64)
    ext = v[:, ry][:, :, rx].reshape(B, gy, th, gx, tw).transpose(0, 1, 3, 2, 4).reshape(B * gy * gx, th * tw)
    keys = ext.astype(np.int64) + 256 * np.arange(B * gy * gx, dtype=np.int64)[:, None]
    return np.bincount(keys.reshape(-1), minlength=B * gy * gx * 256).reshape(B, gy, gx, 256)


def redistribute(h, cl):
    """the clipped histograms with the excess put back (cl == 0: unchanged)"""
    h = h.astype(np.int64).copy()
    if cl <= 0:
        return h
    clipped = np.maximum(h - cl, 0).sum(-1, keepdims=True)
    h = np.minimum(h, cl)
    batch = clipped // 256
    residual = clipped - 256 * batch
    h += batch
    step = np.maximum(256 // np.maximum(residual, 1), 1)
    i = np.arange(256, dtype=np.int64)
    return h + ((residual > 0) & (i % step == 0) & (i // step < residual))


def lut_of(h, area):
    S = np.cumsum(h, axis=-1).astype(np.int32).astype(F)
    scale = F(255.0) / F(area)
    return np.clip(np.rint(S * scale), 0, 255).astype(np.uint8)


def tables(v, gy, gx, clip_limit):
    """-> (B, gy, gx, 256) uint8 tables of the plane v (B, H, W)"""
    _he, _we, th, tw = geometry(v.shape[1], v.shape[2], gy, gx)
    return lut_of(redistribute(histograms(v, gy, gx), clip_value(clip_limit, th * tw)), th * tw)


def fma(a, b, c):
    """a * b + c with one rounding to float32 at the end (the product of two float32 is exact in float64)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def axis_weights(n, t, g, fused):
    """-> (i1, i2, a, a1) of the n pixels of an axis with tile side t and g tiles"""
    p = np.arange(n).astype(F)
    inv = F(1.0) / F(t)
    f = fma(p, np.full(n, inv, F), np.full(n, -0.5, F)) if fused else p * inv - F(0.5)
    i1 = np.floor(f)
    a = f - i1
    a1 = F(1.0) - a
    i1 = i1.astype(np.int64)
    return np.maximum(i1, 0), np.minimum(i1 + 1, g - 1), a.astype(F), a1.astype(F)


def blend(v, luts, fused=False):
    """v: (B, H, W) integers, luts (B, gy, gx, 256) -> (B, H, W) uint8.  fused: every a * b + c is rounded once (what a compiler that
    contracts multiply-adds would compute): a wrong reading of the definition, kept for the tests that show the cases can tell."""
    B, H, W = v.shape
    gy, gx = luts.shape[1], luts.shape[2]
    _he, _we, th, tw = geometry(H, W, gy, gx)
    y1, y2, ya, ya1 = axis_weights(H, th, gy, fused)
    x1, x2, xa, xa1 = axis_weights(W, tw, gx, fused)
    bb = np.arange(B)[:, None, None]
    vv = v.astype(np.int64)
    lf = luts.astype(F)

    def g(yi, xi):
        return lf[bb, yi[None, :, None], xi[None, None, :], vv]

    l11, l12, l21, l22 = g(y1, x1), g(y1, x2), g(y2, x1), g(y2, x2)
    xa, xa1 = np.broadcast_to(xa[None, None, :], v.shape), np.broadcast_to(xa1[None, None, :], v.shape)
    ya, ya1 = np.broadcast_to(ya[None, :, None], v.shape), np.broadcast_to(ya1[None, :, None], v.shape)
    if fused:
        top, bot = fma(l11, xa1, l12 * xa), fma(l21, xa1, l22 * xa)
        res = fma(top, ya1, bot * ya)
    else:
        top, bot = l11 * xa1 + l12 * xa, l21 * xa1 + l22 * xa
        res = top * ya1 + bot * ya
    assert res.dtype == F
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def clahe(img, grid_y, grid_x, clip_limit, fused=False):
    """img: (B, H, W, 1 | 3) uint8 -> (the equalised images, the (B, grid_y, grid_x, 256) uint8 tables)"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] in (1, 3)
    if a.shape[3] == 1:
        v = a[..., 0].astype(np.int64)
        luts = tables(v, grid_y, grid_x, clip_limit)
        return blend(v, luts, fused)[..., None], luts
    Y, U, V = rgb2yuv(a)
    luts = tables(Y, grid_y, grid_x, clip_limit)
    return yuv2rgb(blend(Y, luts, fused).astype(np.int64), U, V), luts
