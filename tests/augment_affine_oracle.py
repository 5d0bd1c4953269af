"""numpy restatement of mgu_augment_affine_color (include/mgunet.h, "scale, crop and colour augmentation"): int64 throughout,
vectorised over the output pixels of one image.  It takes the integer parameter table {a0..a5, A row-major, k}, so equality with the
device does not depend on anyone's libm.  `variant` names one wrong reading of the definition (VARIANTS); the host test shows that
the shared cases tell each of them from the definition."""
import numpy as np

VARIANTS = ("blend_no_round", "frac_rounded", "mask_no_round", "clamp_edge", "A_transposed", "mean_over_crop", "shift_toward_zero",
            "a1_a3_swapped", "int32_wrap")
LUMA = (77, 150, 29)


def luma_sum(img_rgb) -> int:
    """S = sum over the pixels of (77 R + 150 G + 29 B) of one (Hs, Ws, 3) RGB image"""
    v = img_rgb.astype(np.int64)
    return int((LUMA[0] * v[..., 0] + LUMA[1] * v[..., 1] + LUMA[2] * v[..., 2]).sum())


def mean_q8(S: int, n: int) -> int:
    return (int(S) + int(n) // 2) // int(n)


def _shr(v, n, variant):
    if variant == "shift_toward_zero":
        return np.where(v >= 0, v >> n, -((-v) >> n))
    return v >> n


def coordinates(row, out_hw, variant=None):
    """(sx, sy) int64 (H, W): 16.16 source coordinates of every output pixel"""
    a0, a1, a2, a3, a4, a5 = (int(v) for v in row[:6])
    if variant == "a1_a3_swapped":
        a1, a3 = a3, a1
    y, x = np.mgrid[0:int(out_hw[0]), 0:int(out_hw[1])].astype(np.int64)
    sx, sy = a2 + y * a1 + x * a0, a5 + y * a4 + x * a3
    if variant == "int32_wrap":
        sx, sy = ((sx + 2 ** 31) % 2 ** 32) - 2 ** 31, ((sy + 2 ** 31) % 2 ** 32) - 2 ** 31
    return sx, sy


def sample_image(img_rgb, row, out_hw, fill=(0, 0, 0), variant=None):
    """the bilinear bytes v (H, W, 3) int64 before the colour step"""
    Hs, Ws = img_rgb.shape[:2]
    src = img_rgb.astype(np.int64)
    sx, sy = coordinates(row, out_hw, variant)
    if variant == "frac_rounded":
        sx, sy = sx + 128, sy + 128
    ix, iy = _shr(sx, 16, variant), _shr(sy, 16, variant)
    fx, fy = _shr(sx, 8, variant) & 255, _shr(sy, 8, variant) & 255
    fillv = np.asarray(fill, np.int64)

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
        xc, yc = np.clip(xx, 0, Ws - 1), np.clip(yy, 0, Hs - 1)
        if variant == "clamp_edge":
            return src[yc, xc]
        return np.where(inside[..., None], src[yc, xc], fillv)

    acc = ((256 - fx) * (256 - fy))[..., None] * tap(ix, iy) + (fx * (256 - fy))[..., None] * tap(ix + 1, iy) \
        + ((256 - fx) * fy)[..., None] * tap(ix, iy + 1) + (fx * fy)[..., None] * tap(ix + 1, iy + 1)
    return (acc + (0 if variant == "blend_no_round" else 32768)) >> 16


def interior(img_hw, row, out_hw):
    """bool (H, W): all four taps of the pixel lie inside the source"""
    sx, sy = coordinates(row, out_hw)
    ix, iy = sx >> 16, sy >> 16
    return (ix >= 0) & (ix + 1 < img_hw[1]) & (iy >= 0) & (iy + 1 < img_hw[0])


def sample_mask(mask, row, out_hw, mask_fill=-100, num_classes=0, variant=None):
    Hs, Ws = mask.shape
    sx, sy = coordinates(row, out_hw, variant)
    half = 0 if variant == "mask_no_round" else 32768
    mx, my = _shr(sx + half, 16, variant), _shr(sy + half, 16, variant)
    inside = (mx >= 0) & (mx < Ws) & (my >= 0) & (my < Hs)
    v = mask.astype(np.int64)[np.clip(my, 0, Hs - 1), np.clip(mx, 0, Ws - 1)]
    if num_classes > 0:
        v = np.clip(v, 0, num_classes - 1)
    return np.where(inside, v, np.int64(mask_fill))


def colour(v, row, m, variant=None):
    """the colour step on sampled bytes v (H, W, 3) int64 with the source's mean luma m (Q8) -> bytes (H, W, 3) int64"""
    A = np.asarray([int(t) for t in row[6:15]], np.int64).reshape(3, 3)
    if variant == "A_transposed":
        A = A.T
    k = int(row[15])
    if variant == "mean_over_crop":
        m = mean_q8(luma_sum(v), v.shape[0] * v.shape[1])
    t = _shr(np.int64(k * int(m) + 128), 8, variant)
    q = v @ A.T + t + 2048
    return np.clip(_shr(q, 12, variant), 0, 255)


def normalize(bytes_hw3, mean, std):
    """ToTensor (/255) and Normalize in float32, -> (3, H, W) float32"""
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    v = bytes_hw3.astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(((v - m) / s).astype(np.float32).transpose(2, 0, 1))


def augment(images_u8, table, out_hw, mean, std, masks=None, fill=(0, 0, 0), mask_fill=-100, num_classes=0, bgr=False, variant=None):
    """images_u8 (B, Hs, Ws, 3) uint8, table (B, 16) ints, masks optional (B, Hs, Ws) uint8
    -> (out float32 (B, 3, H, W), bytes uint8 (B, H, W, 3) after the colour step, sampled bytes before it, masks int64 (B, H, W) | None)"""
    images_u8, table = np.asarray(images_u8), np.asarray(table).astype(np.int64)
    B, Hs, Ws, _ = images_u8.shape
    outs, byts, smp, ms = [], [], [], []
    for b in range(B):
        rgb = images_u8[b][..., ::-1] if bgr else images_u8[b]
        row = table[b].tolist()
        v = sample_image(rgb, row, out_hw, fill, variant)
        q = colour(v, row, mean_q8(luma_sum(rgb), Hs * Ws), variant)
        smp.append(v.astype(np.uint8)), byts.append(q.astype(np.uint8)), outs.append(normalize(q, mean, std))
        if masks is not None:
            ms.append(sample_mask(np.asarray(masks)[b], row, out_hw, mask_fill, num_classes, variant))
    return np.stack(outs), np.stack(byts), np.stack(smp), (np.stack(ms) if masks is not None else None)


def bilinear_f64(img_rgb, row, out_hw):
    """float64 bilinear sample at (sx, sy) / 65536, unrounded; meaningful on interior() pixels only -> (H, W, 3) float64"""
    Hs, Ws = img_rgb.shape[:2]
    src = img_rgb.astype(np.float64)
    sx, sy = coordinates(row, out_hw)
    u, v = sx.astype(np.float64) / 65536.0, sy.astype(np.float64) / 65536.0
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = (u - x0)[..., None], (v - y0)[..., None]
    g = lambda xx, yy: src[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)]
    return (1 - fx) * (1 - fy) * g(x0, y0) + fx * (1 - fy) * g(x0 + 1, y0) + (1 - fx) * fy * g(x0, y0 + 1) + fx * fy * g(x0 + 1, y0 + 1)
