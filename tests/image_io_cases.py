"""Deterministic cases, references and named wrong variants for the image input / output kernels (csrc/imageops.hip, the integer
arithmetic of csrc/imgmath.h).  Plain numpy / torch / PIL / scipy on the CPU: no fixture, no GPU.  Imported by
tests/test_image_io_cases_host.py (each reference against its independent counterpart, each adversarial case's property with its
count, each wrong variant shown to differ; no GPU) and tests/test_gpu_image_io.py (the kernels against the same references).

What is independent and what is not:
  * PIL resample: the reference is PIL itself (O.preprocess_image calls Image.resize).  pil_resample() restates ImagingResample only to
    carry the wrong variants.
  * Sobel: O.sobel_edges is checked against scipy.ndimage.sobel(mode="mirror") and, for the normalisation, against the exact integer
    rule sobel_exact() (the largest k with k^2 M <= 255^2 m).
  * fp32 bilinear resize: resize_reference() is checked against F.interpolate on the CPU in float64 and float32.
  * patch means, colour map, gather: exact integer / copy semantics, stated here from the definition.
  * cv2 is not installed, so the colour conversions (RGB2GRAY, RGB2YUV, YUV2RGB), cv::equalizeHist and cv::resize(INTER_NEAREST) stay
    pinned only to the oracle's restatement of OpenCV's documented fixed-point code (see the note above preprocess_image in
    oracle/mgunet_oracle.py).  For these the cases are inputs on which a subtly different kernel cannot survive, and every such
    subtle difference is written down below as a variant and shown by the host test to change the output.

Two properties an earlier reading of the arithmetic expected do not exist, and the host test pins that instead:
  * U of RGB2YUV never saturates: 0.492 (B - Y) lies in [-112, 112] for 8-bit input, so only V's two clips can be hit.
  * PIL's BILINEAR (triangle) weights are never negative, so rounding the coefficients with +0.5 "regardless of sign" is the same
    function; the variant is kept, shown to differ from PIL on a BICUBIC resize (negative lobes), and shown to be unreachable here.
  * A window that starts at floor(center - support) instead of int(center - support + 0.5) only gains taps of weight zero (the triangle
    vanishes outside its support): the same function again.  The variant that does change bytes drops the + 0.5 at BOTH ends.
And one rule above ImagingResample: Image.resize (the Python method torchvision's Resize calls; Pillow 12 here) shrinks the height of an
image more than 100 times taller than wide BEFORE the horizontal pass.  (1080, 3) -> (2, 2) is such an image; the variant
horizontal_always, which is what preprocess_resize_u8 did until this case existed, differs from PIL on it."""
import math
from functools import lru_cache

import numpy as np
import torch

import mgunet_oracle as O

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _rng(*key):
    return np.random.RandomState(sum((i + 1) * int(k) for i, k in enumerate(key)) % (2 ** 31))


# ---- 1. PIL resample + normalise ----------------------------------------------------------------------------------------------------------
RESAMPLE_PAIRS = [((1, 1), (5, 7)), ((7, 5), (1, 1)), ((1, 300), (4, 4)), ((2, 3), (64, 64)), ((1080, 3), (2, 2)), ((5, 5), (5, 9)),
                  ((9, 5), (5, 5)), ((64, 64), (64, 64)), ((97, 61), (33, 127))]
RESAMPLE_CONTENTS = ["zeros", "full", "checker", "corners", "noise"]
RESAMPLE_LAYOUTS = ["bgr", "rgb", "grey"]


def resample_image(content: str, src, layout: str) -> np.ndarray:
    """(H, W, 3) uint8, or (H, W) for the grey layout"""
    H, W = src
    C = 1 if layout == "grey" else 3
    if content == "zeros":
        a = np.zeros((H, W, C), np.uint8)
    elif content == "full":
        a = np.full((H, W, C), 255, np.uint8)
    elif content == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        a = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], C, axis=2)
    elif content == "corners":
        a = np.zeros((H, W, C), np.uint8)
        a[0, 0] = a[0, W - 1] = a[H - 1, 0] = a[H - 1, W - 1] = 255
    elif content == "noise":
        a = _rng(H, W, C, 17).randint(0, 256, (H, W, C)).astype(np.uint8)
    else:
        raise KeyError(content)
    return a[:, :, 0].copy() if layout == "grey" else a


def resample_reference(img: np.ndarray, dst, layout: str) -> torch.Tensor:
    """real PIL + ToTensor + Normalize in fp32: (3, H, W) float32"""
    return O.preprocess_image(img, dst, MEAN, STD, bgr=(layout == "bgr"))


PIL_BITS = 32 - 8 - 2
RESAMPLE_VARIANTS = ["vertical_first", "horizontal_always", "round_plus_half", "floor_start", "no_round_window", "no_half"]


def _filter(name, x):
    x = abs(x)
    if name == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    a = -0.5                                                     # PIL's BICUBIC
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_coeffs(in_size: int, out_size: int, variant=None, filt="bilinear"):
    """precompute_coeffs + normalize_coeffs_8bpc of libImaging/Resample.c -> (bounds [(first, count)], int coefficient rows)"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = (1.0 if filt == "bilinear" else 2.0) * filterscale
    ss = 1.0 / filterscale
    bounds, rows = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        if variant == "floor_start":                             # an earlier start only adds taps of weight zero: the same function
            xmin = int(math.floor(center - support))
        else:
            xmin = int(center - support) if variant == "no_round_window" else int(center - support + 0.5)
        xmin = max(xmin, 0)
        xmax = min(int(center + support) if variant == "no_round_window" else int(center + support + 0.5), in_size) - xmin
        k = [_filter(filt, (x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = sum(k)
        k = [v / ww if ww != 0.0 else v for v in k]
        if variant == "round_plus_half":
            rows.append([int(0.5 + v * (1 << PIL_BITS)) for v in k])
        else:
            rows.append([int(-0.5 + v * (1 << PIL_BITS)) if v < 0 else int(0.5 + v * (1 << PIL_BITS)) for v in k])
        bounds.append((xmin, xmax))
    return bounds, rows


def _pil_pass(a: np.ndarray, axis: int, out_size: int, variant, filt):
    bounds, rows = pil_coeffs(a.shape[axis], out_size, variant, filt)
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((out_size,) + a.shape[1:], np.int64)
    half = 0 if variant == "no_half" else 1 << (PIL_BITS - 1)
    for o, ((first, cnt), kk) in enumerate(zip(bounds, rows)):
        acc = np.full(a.shape[1:], half, np.int64)
        for t in range(cnt):
            acc = acc + a[first + t] * kk[t]
        out[o] = np.clip(acc >> PIL_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def pil_resample(img: np.ndarray, dst, variant=None, filt="bilinear") -> np.ndarray:
    """Image.resize on 8-bit channels restated: ImagingResample's horizontal pass, then its vertical one, each only where the size
    changes -- except that Image.resize itself shrinks the height of a tall, narrow image first (height > 100 width).
    variant: None (PIL) | vertical_first (always) | horizontal_always | round_plus_half | floor_start | no_round_window (neither end of the
    window gets the + 0.5: the last live tap is lost) | no_half"""
    a = img[:, :, None] if img.ndim == 2 else img
    H, W = int(dst[0]), int(dst[1])
    tall = a.shape[0] > a.shape[1] * 100 and H < a.shape[0] and variant != "horizontal_always"
    order = [(0, H), (1, W)] if variant == "vertical_first" or tall else [(1, W), (0, H)]
    for axis, n in order:
        if a.shape[axis] != n:
            a = _pil_pass(a, axis, n, variant, filt)
    return a[:, :, 0] if img.ndim == 2 else a


def pil_resize_u8(img: np.ndarray, dst, filt="bilinear") -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(img)).resize((int(dst[1]), int(dst[0])),
                                                                        Image.BILINEAR if filt == "bilinear" else Image.BICUBIC))


# ---- 2. mask resize -----------------------------------------------------------------------------------------------------------------------
# (src, dst): the 7k -> 9k family (539 = 7 * 77, 693 = 9 * 77 and 77 -> 99; 42 -> 54 on the other axis), 3x up, 3x down, 1 -> N, N -> 1, equal
MASK_PAIRS = [((539, 77), (693, 99)), ((21, 42), (27, 54)), ((100, 100), (300, 300)), ((300, 300), (100, 100)), ((6, 6), (34, 34)),
              ((1, 1), (9, 13)), ((9, 13), (1, 1)), ((1, 17), (5, 1)), ((31, 29), (31, 29))]
MASK_CLASSES = [1, 2, 3, 256]
MASK_VARIANTS = ["float32", "exact"]


def mask_image(src) -> np.ndarray:
    """every value 0..255 present (where the size allows), rows and columns all different, so a source index off by one shows"""
    H, W = src
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy * 37 + xx * 101 + (yy * xx) % 7) % 256).astype(np.uint8)


def mask_index(src_n: int, dst_n: int, variant=None) -> np.ndarray:
    """the source index of every destination index along one axis"""
    x = np.arange(dst_n)
    if variant == "exact":
        return np.minimum(x * src_n // dst_n, src_n - 1)
    if variant == "float32":
        inv = np.float32(1.0) / (np.float32(dst_n) / np.float32(src_n))
        return np.minimum(np.floor(x.astype(np.float32) * inv).astype(np.int64), src_n - 1)
    return np.minimum(np.floor(x * (1.0 / (dst_n / src_n))).astype(np.int64), src_n - 1)   # cv::resize: inv_scale = dsize / ssize in double


def mask_variant(mask: np.ndarray, dst, num_classes: int, variant=None) -> np.ndarray:
    sy, sx = mask_index(mask.shape[0], int(dst[0]), variant), mask_index(mask.shape[1], int(dst[1]), variant)
    return np.clip(mask[sy][:, sx].astype(np.int64), 0, num_classes - 1)


# ---- 3. Sobel -----------------------------------------------------------------------------------------------------------------------------
def grey3(g: np.ndarray) -> np.ndarray:
    return np.repeat(np.asarray(g, np.uint8)[:, :, None], 3, axis=2)


@lru_cache(maxsize=None)
def tie_dense() -> np.ndarray:
    """grey columns 0,0,0,k,k,k for k = 0..255 and a closing 0,0,0, 8 rows (12312 pixels): every gradient is 0 or 4k, the largest 1020,
    so sqrt(m) / max * 255 is the integer k at every pixel"""
    cols = np.concatenate([np.array([0, 0, 0, k, k, k]) for k in range(256)] + [np.zeros(3, np.int64)])
    return grey3(np.tile(cols[None, :], (8, 1)))


CUBE_LEVELS = np.concatenate([np.arange(0, 255, 5), [255]])     # 52 levels, step 5, 255 included


@lru_cache(maxsize=None)
def colour_cube() -> np.ndarray:
    """every RGB triple of the 52-level grid as one (52, 2704, 3) image: r along the rows, (g, b) along the columns"""
    L = CUBE_LEVELS.size
    r, g, b = np.meshgrid(CUBE_LEVELS, CUBE_LEVELS, CUBE_LEVELS, indexing="ij")
    return np.stack([r, g, b], axis=-1).reshape(L, L * L, 3).astype(np.uint8)


SOBEL_BLOCK_SHAPE = (64, 128)     # 8192 pixels = 256 * 8 * 4: 32 blocks of 256 pixels, one per block of the launch


@lru_cache(maxsize=None)
def sobel_last_block() -> np.ndarray:
    """low-contrast noise everywhere (every block has a non-zero local maximum) and a bright bar in the bottom row, whose gradients
    reach only the last two rows = the last 256 pixels = the last block of the launch"""
    H, W = SOBEL_BLOCK_SHAPE
    a = _rng(H, W, 3).randint(0, 24, (H, W, 3)).astype(np.uint8)
    a[H - 1, 40:72] = (255, 250, 245)
    return a


def sobel_single_gradient() -> np.ndarray:
    """an odd pixel inside a flat image lights its eight neighbours; on a one-pixel-wide column gx is zero and gy(y) = 4 (g[y+1] - g[y-1])
    with reflect-101 ends, so an odd TOP pixel gives exactly one nonzero gradient, at row 1 (the host test counts it)"""
    a = np.full((5, 1, 3), 200, np.uint8)
    a[0, 0] = 201
    return a


@lru_cache(maxsize=None)
def sobel_cases() -> dict:
    """name -> (H, W, 3) uint8"""
    cases = {}
    for H, W in ((1, 1), (1, 9), (9, 1), (2, 2), (2, 7), (3, 3), (37, 45)):
        cases[f"noise_{H}x{W}"] = _rng(H, W, 3, 5).randint(0, 256, (H, W, 3)).astype(np.uint8)
    cases["flat_0"] = np.zeros((6, 10, 3), np.uint8)
    cases["flat_255"] = np.full((6, 10, 3), 255, np.uint8)
    cases["flat_colour"] = np.tile(np.array([[[13, 200, 77]]], np.uint8), (7, 5, 1))
    cases["single_gradient"] = sobel_single_gradient()
    cases["last_block"] = sobel_last_block()
    # found by search over seeds: two pixels where 255 sqrt(m / M) lies within float32's error of an integer without being one
    cases["near_tie"] = np.random.RandomState(126).randint(0, 256, (32, 32, 3)).astype(np.uint8)
    cases["tie_dense"] = tie_dense()
    cases["cube"] = colour_cube()
    return cases


SOBEL_VARIANTS = ["reflect", "grey14", "round", "float32"]


def cv_gray(rgb: np.ndarray, bits: int = 15) -> np.ndarray:
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    if bits == 15:
        return (r * 9798 + g * 19235 + b * 3735 + (1 << 14)) >> 15
    return (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14


def sobel_mag2(rgb: np.ndarray, variant=None) -> np.ndarray:
    """squared 3x3 Sobel magnitude in exact integers"""
    g = np.pad(cv_gray(rgb, 14 if variant == "grey14" else 15), 1, mode="symmetric" if variant == "reflect" else "reflect")
    gx = (g[:-2, 2:] + 2 * g[1:-1, 2:] + g[2:, 2:]) - (g[:-2, :-2] + 2 * g[1:-1, :-2] + g[2:, :-2])
    gy = (g[2:, :-2] + 2 * g[2:, 1:-1] + g[2:, 2:]) - (g[:-2, :-2] + 2 * g[:-2, 1:-1] + g[:-2, 2:])
    return gx * gx + gy * gy


def sobel_exact(rgb: np.ndarray) -> np.ndarray:
    """floor(255 sqrt(m / M)) without floating point: the largest k with k^2 M <= 255^2 m"""
    m = sobel_mag2(rgb)
    M = int(m.max())
    if M == 0:
        return np.zeros(m.shape, np.uint8)
    q = (m * 65025) // M                                          # floor(sqrt(floor(x))) = floor(sqrt(x))
    k = np.floor(np.sqrt(q.astype(np.float64))).astype(np.int64)
    k = np.where(k * k > q, k - 1, k)
    k = np.where((k + 1) * (k + 1) <= q, k + 1, k)
    assert np.all(k * k <= q) and np.all((k + 1) * (k + 1) > q)
    return k.astype(np.uint8)


def sobel_variant(rgb: np.ndarray, variant=None) -> np.ndarray:
    m = sobel_mag2(rgb, variant)
    if m.max() == 0:
        return np.zeros(m.shape, np.uint8)
    if variant == "float32":
        mag = np.sqrt(m.astype(np.float32))
        return (mag / mag.max() * np.float32(255)).astype(np.uint8)
    mag = np.sqrt(m.astype(np.float64))
    v = mag / mag.max() * 255
    return (np.rint(v) if variant == "round" else v).astype(np.uint8)


# ---- 4. histogram equalisation --------------------------------------------------------------------------------------------------------------
def grey_from_counts(counts: dict, shape) -> np.ndarray:
    """a grey RGB image (Y = the grey level, U = V = 128) with counts[level] pixels of each level, levels interleaved"""
    v = np.concatenate([np.full(n, lvl, np.int64) for lvl, n in sorted(counts.items())])
    assert v.size == shape[0] * shape[1], (v.size, shape)
    return grey3(v[_rng(v.size, 3).permutation(v.size)].reshape(shape))


def half_tie_counts() -> dict:
    """2 pixels of level 0 (the first non-empty bin), then 510 more: 1 of level 1, 2 of each level 2..254, 3 of level 255.  scale = 255 /
    510 = 0.5 exactly and the cumulative sum is odd at levels 1..254: each table entry there is k + 1/2"""
    c = {0: 2, 1: 1, 255: 3}
    c.update({lvl: 2 for lvl in range(2, 255)})
    return c


def scale_probe_counts() -> dict:
    """2 pixels of level 0, then 210 more with the cumulative sums 21, 49, 77, 105, 161, 189, 210 at levels 10, 20, .. 70.  255 / 210 is
    no float: 255 s / 210 is k + 1/2 in exact arithmetic at the first six sums, and float(s) * (255.f / 210.f) rounds to the other side of
    the tie than double s * (255.0 / 210.0) at each of them (found by search over the totals below 6000; the host test asserts it)"""
    return {0: 2, 10: 21, 20: 28, 30: 28, 40: 28, 50: 56, 60: 28, 70: 21}


@lru_cache(maxsize=None)
def histeq_cases() -> dict:
    """name -> (H, W, 3) uint8"""
    cases = {"cube": colour_cube(), "tie_dense": tie_dense(), "last_block": sobel_last_block()}
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    cases["corners"] = np.tile(corners[None, :, :], (3, 1, 1)) // np.array([1, 1, 2], np.uint8)[:, None, None]   # two full rows, one at half level
    cases["half_ties"] = grey_from_counts(half_tie_counts(), (8, 64))
    cases["scale_probe"] = grey_from_counts(scale_probe_counts(), (4, 53))
    cases["constant"] = np.tile(np.array([[[200, 30, 90]]], np.uint8), (5, 9, 1))
    cases["two_levels"] = grey_from_counts({40: 30, 41: 33}, (7, 9))
    cases["all_but_one"] = grey_from_counts({17: 62, 200: 1}, (7, 9))
    cases["noise_37x45"] = sobel_cases()["noise_37x45"]
    return cases


HISTEQ_BIG_SHAPE = (1024, 2048)    # 2 097 152 pixels = 1024 blocks * 256 threads * 8: the capped histogram launch strides 8 times


@lru_cache(maxsize=None)
def histeq_big() -> np.ndarray:
    H, W = HISTEQ_BIG_SHAPE
    a = _rng(H, W, 9).randint(0, 256, (H, W, 3)).astype(np.uint8)
    a[: H // 2, : W // 2] //= 4
    a[H // 2:, : W // 3] = (a[H // 2:, : W // 3] // 3 + 150).astype(np.uint8)
    return a


HISTEQ_VARIANTS = ["half_up", "scale_double", "cumsum_with_i0", "uv_unsaturated"]


def yuv_preclip(rgb: np.ndarray):
    """Y and the U, V of cv2.COLOR_RGB2YUV BEFORE saturation"""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    Y = (r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14
    U = ((b - Y) * 8061 + (128 << 14) + (1 << 13)) >> 14
    V = ((r - Y) * 14369 + (128 << 14) + (1 << 13)) >> 14
    return Y, U, V


def equalize_table(hist: np.ndarray, variant=None) -> np.ndarray:
    hist = np.asarray(hist, np.int64)
    total = int(hist.sum())
    i0 = int(np.nonzero(hist)[0][0])
    if hist[i0] == total:
        return np.full(256, i0, np.int64)
    lut = np.zeros(256, np.int64)
    s = int(hist[i0]) if variant == "cumsum_with_i0" else 0
    scale32 = np.float32(255.0) / np.float32(total - hist[i0])
    scale64 = 255.0 / float(total - hist[i0])
    for i in range(i0 + 1, 256):
        s += int(hist[i])
        v = float(s) * scale64 if variant == "scale_double" else np.float32(s) * scale32
        r = math.floor(float(v) + 0.5) if variant == "half_up" else np.rint(v)
        lut[i] = min(max(int(r), 0), 255)
    return lut


def equalize_variant(rgb: np.ndarray, variant=None) -> np.ndarray:
    Y, U, V = yuv_preclip(rgb)
    if variant != "uv_unsaturated":
        U, V = np.clip(U, 0, 255), np.clip(V, 0, 255)
    Y2 = equalize_table(np.bincount(Y.reshape(-1), minlength=256), variant)[Y]
    u, v = U - 128, V - 128

    def descale(t):
        return (t + (1 << 13)) >> 14
    out = np.stack([Y2 + descale(v * 18678), Y2 + descale(u * -6472 + v * -9519), Y2 + descale(u * 33292)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


# ---- 5. patch means, colour map, gather -----------------------------------------------------------------------------------------------------
def patch_mean_exact(img: np.ndarray, patch: int, per_channel: bool) -> torch.Tensor:
    """exact integer sums of every (zero padded) patch, divided in float64 by the patch's full size, rounded once to fp32"""
    a = img[:, :, None] if img.ndim == 2 else img
    H, W, C = a.shape
    nph, npw = -(-H // patch), -(-W // patch)
    out = np.zeros((nph * npw, C if per_channel else 1), np.float64)
    for py in range(nph):
        for px in range(npw):
            blk = a[py * patch:(py + 1) * patch, px * patch:(px + 1) * patch].astype(np.int64)
            s = blk.sum(axis=(0, 1))
            out[py * npw + px] = (s / (float(patch) * patch)) if per_channel else (int(s.sum()) / (float(patch) * patch * C))
    return torch.from_numpy(out.astype(np.float32))


# (H, W, C, patch): patch 1; patch larger than the image; patch 4096 on a small image; H and W no multiples of the patch; 1, 3, 4 channels
PATCH_MEAN_CASES = [(5, 7, 3, 1), (5, 7, 1, 16), (9, 6, 4, 4096), (37, 45, 3, 16), (37, 45, 1, 8), (33, 18, 4, 5), (40, 56, 3, 32)]
PATCH_MEAN_FULL = (1500, 1500, 4, 2048)   # all 255, one patch: the sum 2 295 000 000 lies between 2^31 and 2^32
PATCH_MEAN_WIDE = (4096, 3)               # all 255, side = patch = 4096 (the entry point's limit), 3 channels: the sum exceeds 2^32


def patch_mean_image(H, W, C, full=False) -> np.ndarray:
    if full:
        return np.full((H, W, C), 255, np.uint8)
    return _rng(H, W, C, 23).randint(0, 256, (H, W, C)).astype(np.uint8)


def colorize_reference(labels: np.ndarray, num_classes: int, palette: np.ndarray):
    """-> (colour map, uint8 label map): labels outside [0, num_classes) stay black; the label map is labels.astype(uint8)"""
    return O.colorize_labels(labels, num_classes, [tuple(int(v) for v in row) for row in palette]), labels.astype(np.uint8)


def palette_for(num_classes: int) -> np.ndarray:
    k = np.arange(num_classes)
    return np.stack([(k * 7 + 1) % 256, (k * 13 + 2) % 256, 255 - k % 256], axis=1).astype(np.uint8)   # no row is black


def gather_reference(table: np.ndarray, ids: np.ndarray) -> np.ndarray:
    out = np.zeros(ids.shape + (table.shape[1],), np.float32)
    ok = (ids >= 0) & (ids < table.shape[0])
    out[ok] = table[ids[ok]]
    return out


# ---- 6. fp32 bilinear resize ------------------------------------------------------------------------------------------------------------------
# (B, Hi, Wi, Ho, Wo, C)
RESIZE_SHAPES = [(1, 1, 1, 5, 7, 4), (2, 7, 9, 24, 40, 4), (2, 24, 40, 7, 9, 8), (1, 5, 11, 5, 11, 12), (1, 12, 20, 24, 40, 16),
                 (1, 33, 17, 1, 1, 4), (1, 3, 500, 9, 125, 4)]


def resize_input(B, Hi, Wi, C, integers=False) -> np.ndarray:
    """(B, Hi, Wi, C) float32, NHWC"""
    if integers:
        return _rng(B, Hi, Wi, C).randint(-8, 9, (B, Hi, Wi, C)).astype(np.float32)
    return O.formula_normal("imageio/resize", (B, Hi, Wi, C), seed=Hi * 1000 + Wi).astype(np.float32)


def _resize_axis(n_in: int, n_out: int, coord):
    """aten's area_pixel_compute_scale / _source_index (align_corners = False) in `coord` arithmetic -> (src, i0, i1, lambda1 as float64)"""
    scale = coord(n_in) / coord(n_out)
    src = np.maximum(scale * (np.arange(n_out).astype(coord) + coord(0.5)) - coord(0.5), coord(0))
    assert src.dtype == coord
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    return src, i0, i1, (src - i0.astype(coord)).astype(np.float64)


def resize_reference(x: np.ndarray, Ho: int, Wo: int, coord=np.float32):
    """x (B, Hi, Wi, C) -> (ref64, bar, lo, hi), each (B, Ho, Wo, C): the float64 blend at aten's source coordinates; the per-element bar
        8 * 2^-24 (|a| + |b| + |c| + |d|) + ulp32(src_y) |bottom - top| + ulp32(src_x) |right - left|
    (at most five roundings on any path from an input to the output; a coordinate formed in one fused operation differs by an ulp and
    bilinear is continuous in it); the min / max of the four sources."""
    x64 = x.astype(np.float64)
    sy, y0, y1, ly = _resize_axis(x.shape[1], Ho, coord)
    sx, x0, x1, lx = _resize_axis(x.shape[2], Wo, coord)
    a, b = x64[:, y0][:, :, x0], x64[:, y0][:, :, x1]
    c, d = x64[:, y1][:, :, x0], x64[:, y1][:, :, x1]
    LY, LX = ly[None, :, None, None], lx[None, None, :, None]
    top, bottom = (1 - LX) * a + LX * b, (1 - LX) * c + LX * d
    left, right = (1 - LY) * a + LY * c, (1 - LY) * b + LY * d
    ref = (1 - LY) * top + LY * bottom
    uy = np.spacing(sy.astype(np.float32)).astype(np.float64)[None, :, None, None]
    ux = np.spacing(sx.astype(np.float32)).astype(np.float64)[None, None, :, None]
    bar = 8 * 2.0 ** -24 * (np.abs(a) + np.abs(b) + np.abs(c) + np.abs(d)) + uy * np.abs(bottom - top) + ux * np.abs(right - left)
    four = np.stack([a, b, c, d])
    return ref, bar, four.min(axis=0), four.max(axis=0)
