"""Host-side mirrors of the reference's input / output pipeline, routed through libmgunet.so:

    ImagePreprocessor        preprocessing/image_preprocessing/image_preprocess.py:6-126
    EdgeDetector             preprocessing/graph_feature_processing/edge_detection.py:4-44
    HistogramEqualizer       preprocessing/graph_feature_processing/histogram_equalization.py:4-49
    CLAHE                    (no counterpart: cv2.createCLAHE(clipLimit, tileGridSize).apply as this build defines it)
    GaussianSmoother         preprocessing/graph_feature_processing/gaussian_smoothing.py:4-34
    patch_features_u8        scripts/graph_refinement.py:97-104   (image_to_patches(...).mean(...))
    postprocess_segmentation scripts/infer_segmentation.py:20-51

Same class names, constructor arguments and method names.  The reference works on host numpy arrays with cv2 / PIL; here the
pixels go to the device once (uint8) and every step is a HIP kernel that reproduces the library's integer arithmetic exactly.
Methods accept a numpy array (returned type: what the reference returns) or a uint8 CUDA tensor (returned: CUDA tensors, no host
round trip).  File paths are decoded with PIL (RGB order): cv2 is not a dependency of this package.

ImagePreprocessor(apply_augmentation=True) reproduces the reference's RandomHorizontalFlip(0.5) -> RandomRotation(15) bit for bit: the
host makes torchvision's two draws from torch's generator (draw_flip_rotate) and the device applies PIL's fixed-point NEAREST rotation
(pil_rotation_fixed) inside the ToTensor + Normalize pass.  preprocess_pair applies one draw to an image AND its mask (the reference
augments only the image), and RandomFlipRotate augments a whole device batch in one launch.  RandomAffineColor is this build's
own stage (the reference has none): scale / crop / rotation with bilinear resampling and a colour jitter, from the uint8 batch;
RandomElasticAffineColor adds the U-Net paper's elastic deformation (a cubic B-spline of coarse random displacements) to the same pass
and carries an int32 instance map along."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib

def _device():
    """The current HIP device, where host images are moved."""
    _lib.require_hip(torch.device("cuda" if torch.cuda.is_available() else "cpu"), "mgunet.preprocess")
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev_u8(a):
    """numpy uint8 array | uint8 tensor -> (contiguous uint8 CUDA tensor, came_from_numpy)"""
    if isinstance(a, np.ndarray):
        if a.dtype != np.uint8:
            raise TypeError(f"expected a uint8 image, got {a.dtype}")
        return torch.from_numpy(np.ascontiguousarray(a)).to(_device()), True
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.uint8:
            raise TypeError(f"expected a uint8 image, got {a.dtype}")
        return (a if a.is_cuda else a.to(_device())).contiguous(), False
    raise TypeError("Input must be an image path (str) or a NumPy array.")


_MAX_SIDE = 8192   # PIL rotates larger images through a float64 path that is not reproduced


def pil_rotation_fixed(angle: float, w: int, h: int) -> tuple:
    """The int32 coefficients (a0..a5) PIL's NEAREST affine path (affine_fixed in libImaging/Geometry.c) uses for
    Image.rotate(angle, expand=False, center=None) of a w x h image: output pixel (x, y) reads source pixel
    ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16), or the fill colour when that lies outside the image.  The matrix is built as
    Image.rotate builds it (angle % 360, -radians, cos / sin rounded to 15 digits, centre (w/2, h/2)), then FIX(v) = floor(v 65536 + 0.5)
    with the half-pixel centre folded into a2 / a5.  Sides above 8192 raise: PIL would switch to its float64 path."""
    w, h = int(w), int(h)
    if not (1 <= w <= _MAX_SIDE and 1 <= h <= _MAX_SIDE):
        raise ValueError(f"rotation of a {w} x {h} image: sides must be in [1, {_MAX_SIDE}] (PIL's fixed-point path)")
    cx, cy = w / 2.0, h / 2.0
    r = -math.radians(float(angle) % 360.0)
    m0, m1, m3, m4 = round(math.cos(r), 15), round(math.sin(r), 15), round(-math.sin(r), 15), round(math.cos(r), 15)
    m2 = m0 * -cx + m1 * -cy + 0.0 + cx
    m5 = m3 * -cx + m4 * -cy + 0.0 + cy

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))

    return fix(m0), fix(m1), fix(m2 + m0 * 0.5 + m1 * 0.5), fix(m3), fix(m4), fix(m5 + m3 * 0.5 + m4 * 0.5)


def draw_flip_rotate(p: float = 0.5, degrees: float = 15, generator: torch.Generator = None) -> tuple:
    """One image's draws of RandomHorizontalFlip(p) -> RandomRotation(degrees), in torchvision's order and with its calls:
    flip = torch.rand(1) < p (RandomHorizontalFlip.forward), then angle = float(torch.empty(1).uniform_(-degrees, degrees).item())
    (RandomRotation.get_params); both are drawn for every image.  generator=None draws from torch's global CPU generator, as the
    reference does, and leaves it where those two calls leave it.  -> (bool, float).
    The order and the calls follow torchvision's transforms.py as documented for 0.8 and later (RandomRotation's fill=0 default
    since 0.12 does not change the draws); it has not yet been run side by side with an installed torchvision."""
    d = float(degrees)
    if d < 0:
        raise ValueError("If degrees is a single number, it must be positive.")   # torchvision's _setup_angle
    flip = bool(torch.rand(1, generator=generator) < p)
    angle = float(torch.empty(1).uniform_(-d, d, generator=generator).item())
    return flip, angle


def _load_image(image_path_or_array):
    """-> (device uint8 (H, W, 1 | 3), bgr flag)"""
    bgr = 1                                   # arrays are BGR, as cv2.imread delivers them (:76-78)
    if isinstance(image_path_or_array, str):
        from PIL import Image
        try:
            image = np.asarray(Image.open(image_path_or_array).convert("RGB"))
        except FileNotFoundError:
            raise FileNotFoundError(f"Image not found at {image_path_or_array}")
        bgr = 0
    else:
        image = image_path_or_array
    img, _ = _to_dev_u8(image)
    if img.dim() == 2:
        img = img.unsqueeze(-1)               # grey -> three equal channels (:79-80)
    if img.dim() != 3 or img.shape[2] not in (1, 3):
        raise ValueError("expected an (H, W, 3) or (H, W) uint8 image")
    return img, bgr


def _load_mask(mask_path_or_array):
    if isinstance(mask_path_or_array, str):
        from PIL import Image
        try:
            mask = np.asarray(Image.open(mask_path_or_array).convert("L"))
        except FileNotFoundError:
            raise FileNotFoundError(f"Mask not found at {mask_path_or_array}")
    else:
        mask = mask_path_or_array
        if isinstance(mask, np.ndarray) and mask.ndim == 3:
            mask = mask.squeeze(2) if mask.shape[2] == 1 else np.argmax(mask, axis=2).astype(np.uint8)   # :108-114
    m, _ = _to_dev_u8(mask)
    if m.dim() != 2:
        raise ValueError("expected an (H, W) mask")
    return m


class ImagePreprocessor:
    def __init__(self, resize_dim=(128, 128), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), apply_augmentation=False):
        self.resize_dim = resize_dim  # H, W
        self.mean, self.std = mean, std
        self.apply_augmentation = apply_augmentation
        # image_preprocess.py:44-51: RandomHorizontalFlip(p=0.5) -> RandomRotation(degrees=15) between Resize and ToTensor
        self.flip_p, self.degrees = 0.5, 15

    def _draw(self, augment, generator=None):
        if augment is not None:
            return bool(augment[0]), float(augment[1])
        return draw_flip_rotate(self.flip_p, self.degrees, generator)

    def preprocess(self, image_path_or_array, out: torch.Tensor = None, augment=None):
        """-> (3, H, W) float32 CUDA tensor (or fills `out`, any (3, H, W) view -- e.g. one image of an NHWC batch).
        With apply_augmentation the flip / rotation draws come from torch's global generator exactly as the reference's transforms
        make them; augment=(flip, angle) gives them explicitly instead."""
        if augment is not None and not self.apply_augmentation:
            raise ValueError("augment=(flip, angle) needs apply_augmentation=True")
        img, bgr = _load_image(image_path_or_array)
        Hs, Ws, ch = img.shape
        H, W = int(self.resize_dim[0]), int(self.resize_dim[1])
        if out is None:
            out = torch.empty((3, H, W), device=img.device, dtype=torch.float32)
        elif tuple(out.shape) != (3, H, W) or out.dtype != torch.float32 or out.device != img.device:
            raise ValueError("`out` must be a float32 (3, H, W) view on the image's device")
        if self.apply_augmentation:
            flip, angle = self._draw(augment)
            return self._image_aug(img, bgr, out, flip, angle)
        mean, std = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std)
        _lib.call("mgu_preprocess_image_u8", img.device, img, Hs, Ws, ch, bgr, H, W, mean, std, out, *out.stride())
        return out

    def _image_aug(self, img, bgr, out, flip, angle):
        Hs, Ws, ch = img.shape
        H, W = int(self.resize_dim[0]), int(self.resize_dim[1])
        fix = (C.c_int32 * 6)(*pil_rotation_fixed(angle, W, H))
        mean, std = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std)
        _lib.call("mgu_preprocess_image_u8_aug", img.device, img, Hs, Ws, ch, bgr, H, W, mean, std, out, *out.stride(), int(flip), fix)
        return out

    def preprocess_mask(self, mask_path_or_array, num_classes):
        m = _load_mask(mask_path_or_array)
        H, W = int(self.resize_dim[0]), int(self.resize_dim[1])
        out = torch.empty((H, W), device=m.device, dtype=torch.int64)
        _lib.call("mgu_preprocess_mask_u8", m.device, m, m.shape[0], m.shape[1], H, W, int(num_classes), out)
        return out

    def preprocess_pair(self, image, mask, num_classes, mask_fill=0, generator=None, out: torch.Tensor = None, augment=None):
        """preprocess(image) and preprocess_mask(mask, num_classes) under ONE flip / rotation draw -> ((3, H, W) float32, (H, W) int64).
        The reference's MangoDataset.__getitem__ (utils/mango_dataset.py:58-62) augments the image through `preprocess` but calls
        `preprocess_mask` unaugmented, so with apply_augmentation=True its images and masks no longer line up; here both get the same
        flip and rotation.  Rotated-in mask pixels get mask_fill (-100: ignored by the Trainer's cross entropy).  Draws come from
        `generator` (None: torch's global generator), or augment=(flip, angle); without apply_augmentation neither is transformed."""
        if not self.apply_augmentation:
            if augment is not None:
                raise ValueError("augment=(flip, angle) needs apply_augmentation=True")
            return self.preprocess(image, out=out), self.preprocess_mask(mask, num_classes)
        flip, angle = self._draw(augment, generator)
        img, bgr = _load_image(image)
        m = _load_mask(mask)
        H, W = int(self.resize_dim[0]), int(self.resize_dim[1])
        if out is None:
            out = torch.empty((3, H, W), device=img.device, dtype=torch.float32)
        elif tuple(out.shape) != (3, H, W) or out.dtype != torch.float32 or out.device != img.device:
            raise ValueError("`out` must be a float32 (3, H, W) view on the image's device")
        self._image_aug(img, bgr, out, flip, angle)
        mout = torch.empty((H, W), device=m.device, dtype=torch.int64)
        fix = (C.c_int32 * 6)(*pil_rotation_fixed(angle, W, H))
        _lib.call("mgu_preprocess_mask_u8_aug", m.device, m, m.shape[0], m.shape[1], H, W, int(num_classes), int(flip), fix, int(mask_fill), mout)
        return out, mout


class RandomFlipRotate:
    """RandomHorizontalFlip(p) -> RandomRotation(degrees) (NEAREST, fill black) of a normalised fp32 batch on the device, one launch for
    the images and their masks.  Per image the draws are those of draw_flip_rotate, in batch order, so images[i] comes out bitwise as
    ImagePreprocessor(apply_augmentation=True).preprocess_pair would have made it from the same draws.  Rotated-in pixels get
    `fill` (default: the normalised black (0 - mean) / std in float32) and mask_fill (-100: ignored by the Trainer's cross entropy)."""

    def __init__(self, p=0.5, degrees=15, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), mask_fill=0, fill=None):
        if float(degrees) < 0:
            raise ValueError("If degrees is a single number, it must be positive.")
        self.p, self.degrees, self.mask_fill = p, degrees, int(mask_fill)
        if fill is None:
            fill = (np.float32(0) / np.float32(255) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
        self.fill = tuple(float(v) for v in np.asarray(fill, np.float32).reshape(-1))

    def draw(self, B: int, W: int, H: int, generator=None) -> torch.Tensor:
        """-> (B, 7) int32 host table of {flip, a0..a5}, two draws per image in batch order."""
        rows = []
        for _ in range(B):
            flip, angle = draw_flip_rotate(self.p, self.degrees, generator)
            rows.append((int(flip),) + pil_rotation_fixed(angle, W, H))
        return torch.tensor(rows, dtype=torch.int32).reshape(B, 7)

    def __call__(self, images: torch.Tensor, masks: torch.Tensor = None, generator=None, out: torch.Tensor = None):
        """images: (B, C, H, W) float32 on the device, any strides; masks: optional (B, H, W) int64.  -> augmented images (a new tensor
        with the layout of `images`, or `out`) and, with masks, (images, masks)."""
        if not images.is_cuda or images.dtype != torch.float32 or images.dim() != 4:
            raise TypeError("images must be a (B, C, H, W) float32 tensor on the HIP device")
        B, Cc, H, W = images.shape
        if Cc != len(self.fill):
            raise ValueError(f"{Cc} channels but {len(self.fill)} fill values (mean / std)")
        dev = images.device
        if masks is not None:
            if masks.dtype != torch.int64 or masks.device != dev or tuple(masks.shape) != (B, H, W):
                raise ValueError("masks must be a (B, H, W) int64 tensor on the images' device")
            masks = masks.contiguous()
        if out is None:
            out = torch.empty_like(images)
        elif tuple(out.shape) != (B, Cc, H, W) or out.dtype != torch.float32 or out.device != dev:
            raise ValueError("`out` must be a float32 (B, C, H, W) tensor on the images' device")
        params = self.draw(B, W, H, generator).to(dev)
        mout = torch.empty((B, H, W), device=dev, dtype=torch.int64) if masks is not None else None
        si, so = (C.c_int64 * 4)(*images.stride()), (C.c_int64 * 4)(*out.stride())
        fill = (C.c_float * Cc)(*self.fill)
        _lib.call("mgu_augment_flip_rotate", dev, images, out, B, Cc, H, W, si, so, fill, masks, mout, self.mask_fill, params)
        return (out, mout) if masks is not None else out


def _fix(v: float, bits: int) -> int:
    return int(math.floor(v * float(1 << bits) + 0.5))


def affine_fixed(flip, angle: float, zoom: float, aspect: float, tx: float, ty: float, src_hw, out_hw) -> tuple:
    """The six int32 coefficients (a0..a5) of mgu_augment_affine_color for one image: output pixel (x, y) of the W x H result reads the
    source at (sx, sy) = (a2 + y a1 + x a0, a5 + y a4 + x a3) / 65536 in pixel-index units.  The crop is the largest window of aspect
    (Ws / Hs) * aspect inside the (Ws / zoom) x (Hs / zoom) window (zoom > 1 enlarges the fruit), centred at
    (Ws/2 + tx (Ws/2)(1 - 1/zoom), Hs/2 + ty (Hs/2)(1 - 1/zoom)), tx, ty in [-1, 1]: for zoom >= 1 the unrotated crop stays inside the
    source, for zoom < 1 the source stays inside the frame.  It is stretched over the result, flipped left-right when `flip`, and
    rotated by `angle` degrees counter-clockwise about its centre (cos / sin rounded to 15 digits, as pil_rotation_fixed).  Float64
    matrix M = R(angle) diag(+-crop_w / W, crop_h / H) on offsets from the centres, both half-pixel centres folded into a2 / a5, then
    FIX(v) = floor(v 65536 + 0.5).  Sides above 8192 or coefficients beyond int32 raise."""
    Hs, Ws = int(src_hw[0]), int(src_hw[1])
    H, W = int(out_hw[0]), int(out_hw[1])
    if not (1 <= Hs <= _MAX_SIDE and 1 <= Ws <= _MAX_SIDE and 1 <= H <= _MAX_SIDE and 1 <= W <= _MAX_SIDE):
        raise ValueError(f"affine_fixed: {Hs} x {Ws} -> {H} x {W}: sides must be in [1, {_MAX_SIDE}]")
    z, a = float(zoom), float(aspect)
    if not (z > 0.0 and a > 0.0 and math.isfinite(z) and math.isfinite(a)):
        raise ValueError("affine_fixed: zoom and aspect must be positive")
    cw, ch = (Ws / z, Hs / (z * a)) if a >= 1.0 else (Ws * a / z, Hs / z)
    px, py = (-cw if flip else cw) / W, ch / H
    r = math.radians(float(angle) % 360.0)
    co, si = round(math.cos(r), 15), round(math.sin(r), 15)
    m00, m01, m10, m11 = co * px, -si * py, si * px, co * py
    cx = Ws / 2.0 + float(tx) * (Ws / 2.0) * (1.0 - 1.0 / z)
    cy = Hs / 2.0 + float(ty) * (Hs / 2.0) * (1.0 - 1.0 / z)
    ox, oy = 0.5 - W / 2.0, 0.5 - H / 2.0
    fix = (_fix(m00, 16), _fix(m01, 16), _fix(cx - 0.5 + m00 * ox + m01 * oy, 16),
           _fix(m10, 16), _fix(m11, 16), _fix(cy - 0.5 + m10 * ox + m11 * oy, 16))
    if any(abs(v) >= 2 ** 31 for v in fix):
        raise ValueError(f"affine_fixed: coefficients {fix} do not fit int32 (zoom {z} is too small for these sizes)")
    return fix


_LUMA_W = (77.0 / 256.0, 150.0 / 256.0, 29.0 / 256.0)
COLOR_Q12_LIMIT = 1 << 15


def color_matrix_q12(brightness: float = 1.0, contrast: float = 1.0, saturation: float = 1.0, hue: float = 0.0) -> tuple:
    """The Q12 colour parameters of mgu_augment_affine_color -> (A: 9 ints row-major, k).  A = FIX12(b c (S_s R_h)) with
    S_s = s I + (1 - s) 1 w^T, w = (77, 150, 29) / 256, and R_h the rotation by 2 pi h about the grey axis (1, 1, 1) / sqrt 3;
    k = FIX12(b (1 - c)): contrast pivots on the image's own mean luma.  FIX12(v) = floor(v 4096 + 0.5).  |A| or |k| above 2^15 raise."""
    b, c, s, h = float(brightness), float(contrast), float(saturation), float(hue)
    S = np.asarray([[s * (i == j) + (1.0 - s) * _LUMA_W[j] for j in range(3)] for i in range(3)], np.float64)
    co, si = math.cos(2.0 * math.pi * h), math.sin(2.0 * math.pi * h)
    K = np.asarray([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]], np.float64)
    R = co * np.eye(3) + (1.0 - co) / 3.0 * np.ones((3, 3)) + si / math.sqrt(3.0) * K
    M = (b * c) * (S @ R)
    A = tuple(_fix(float(v), 12) for v in M.reshape(-1))
    k = _fix(b * (1.0 - c), 12)
    if max(abs(v) for v in A + (k,)) > COLOR_Q12_LIMIT:
        raise ValueError(f"color_matrix_q12: |A| and |k| must stay within 2^15 (factors up to 8), got A = {A}, k = {k}")
    return A, k


def luma_sums(images_u8: torch.Tensor, bgr: bool = False) -> torch.Tensor:
    """S[b] = sum over the pixels of image b of (77 R + 150 G + 29 B), int64 (B,) on the device: the integer sums RandomAffineColor's
    contrast pivots on (mean luma m = (S + n/2) // n in Q8 byte units).  images_u8: (B, Hs, Ws, 3) uint8 on the device."""
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise TypeError("images_u8 must be a (B, Hs, Ws, 3) uint8 tensor")
    _lib.require_hip(images_u8, "mgunet.luma_sums")
    images_u8 = images_u8.contiguous()
    B, Hs, Ws, _c = images_u8.shape
    out = torch.empty((B,), device=images_u8.device, dtype=torch.int64)
    _lib.call("mgu_augment_luma_sums", images_u8.device, images_u8, B, Hs, Ws, int(bool(bgr)), out)
    return out


def _log_uniform(lo: float, hi: float, u: float) -> float:
    return math.exp(math.log(lo) + u * (math.log(hi) - math.log(lo)))


class RandomAffineColor:
    """Random scale / aspect / crop / rotation / flip and colour jitter of a uint8 batch on the device, straight into the normalised
    float32 (B, 3, H, W) batch and the int64 (B, H, W) masks Trainer.train_step takes: at most two launches and one fill, no host
    synchronisation (include/mgunet.h, mgu_augment_affine_color: bilinear image, nearest mask, integers only, bitwise equal to
    tests/augment_affine_oracle.py).  Draws, part of the interface: per image, in batch order, one
    torch.rand(10, dtype=torch.float64, generator=g): [0] flip (< p_flip), [1] angle (uniform in +-degrees), [2] zoom (log-uniform in
    scale), [3] aspect (log-uniform in ratio), [4], [5] crop position tx, ty in [-1, 1], [6..8] brightness, contrast, saturation
    (uniform in [1 - a, 1 + a]), [9] hue (uniform in [-a, a]).  A disabled term still consumes its entry.  Source pixels outside the
    image are `fill` (an RGB byte triple, jittered with the rest) and mask_fill (-100: ignored by every loss here)."""

    def __init__(self, size, scale=(0.5, 2.0), ratio=(3 / 4, 4 / 3), degrees=15, p_flip=0.5, brightness=0.2, contrast=0.2, saturation=0.2,
                 hue=0.02, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), fill=(0, 0, 0), mask_fill=-100, num_classes=0, bgr=False):
        self.size = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))   # H, W
        self.scale, self.ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        if not (0.0 < self.scale[0] <= self.scale[1] and 0.0 < self.ratio[0] <= self.ratio[1]):
            raise ValueError("scale and ratio must be positive (lo, hi) ranges")
        if float(degrees) < 0 or min(float(brightness), float(contrast), float(saturation), float(hue)) < 0:
            raise ValueError("degrees and the colour ranges must be non-negative")
        self.degrees, self.p_flip = float(degrees), float(p_flip)
        self.brightness, self.contrast, self.saturation, self.hue = float(brightness), float(contrast), float(saturation), float(hue)
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.fill = tuple(int(v) for v in fill)
        if len(self.fill) != 3 or not all(0 <= v <= 255 for v in self.fill):
            raise ValueError("fill must be three bytes (R, G, B)")
        self.mask_fill, self.num_classes, self.bgr = int(mask_fill), int(num_classes), bool(bgr)

    def row(self, r, src_hw) -> tuple:
        """the 16 table entries of one image from its ten draws r (floats in [0, 1))"""
        r = [float(v) for v in r]
        fix = affine_fixed(r[0] < self.p_flip, (2.0 * r[1] - 1.0) * self.degrees, _log_uniform(*self.scale, r[2]), _log_uniform(*self.ratio, r[3]),
                           2.0 * r[4] - 1.0, 2.0 * r[5] - 1.0, src_hw, self.size)
        A, k = color_matrix_q12(1.0 + (2.0 * r[6] - 1.0) * self.brightness, 1.0 + (2.0 * r[7] - 1.0) * self.contrast,
                                1.0 + (2.0 * r[8] - 1.0) * self.saturation, (2.0 * r[9] - 1.0) * self.hue)
        return fix + A + (k,)

    def draw(self, B: int, src_hw, generator=None) -> torch.Tensor:
        """-> (B, 16) int32 host table {a0..a5, A row-major, k}, one torch.rand(10, float64) per image in batch order."""
        rows = [self.row(torch.rand(10, dtype=torch.float64, generator=generator).tolist(), src_hw) for _ in range(int(B))]
        return torch.tensor(rows, dtype=torch.int32).reshape(int(B), 16)

    def __call__(self, images_u8: torch.Tensor, masks: torch.Tensor = None, generator=None, out: torch.Tensor = None, params: torch.Tensor = None):
        """images_u8: (B, Hs, Ws, 3) uint8 on the device; masks: optional (B, Hs, Ws) uint8.  -> float32 (B, 3, H, W) (a new contiguous
        tensor, or `out` of any strides, e.g. an NHWC-strided view) and, with masks, (images, int64 (B, H, W) masks).  params: an
        explicit (B, 16) int32 table instead of a draw (a host table lets the luma pass be skipped when every k is 0)."""
        if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
            raise TypeError("images_u8 must be a (B, Hs, Ws, 3) uint8 tensor")
        _lib.require_hip(images_u8, "mgunet.RandomAffineColor")
        dev = images_u8.device
        images_u8 = images_u8.contiguous()
        B, Hs, Ws, _c = images_u8.shape
        H, W = self.size
        if masks is not None:
            if masks.dtype != torch.uint8 or masks.device != dev or tuple(masks.shape) != (B, Hs, Ws):
                raise ValueError("masks must be a (B, Hs, Ws) uint8 tensor on the images' device")
            masks = masks.contiguous()
        if out is None:
            out = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
        elif tuple(out.shape) != (B, 3, H, W) or out.dtype != torch.float32 or out.device != dev:
            raise ValueError("`out` must be a float32 (B, 3, H, W) tensor on the images' device")
        if params is None:
            params = self.draw(B, (Hs, Ws), generator)
        if tuple(params.shape) != (B, 16) or params.dtype != torch.int32:
            raise ValueError("params must be a (B, 16) int32 table")
        need_mean = 1 if params.is_cuda else int(bool((params[:, 15] != 0).any()))
        if not params.is_cuda and int(params[:, 6:].abs().max()) > COLOR_Q12_LIMIT:
            raise ValueError("params: |A| and |k| must stay within 2^15")
        params = params.to(dev).contiguous()
        mout = torch.empty((B, H, W), device=dev, dtype=torch.int64) if masks is not None else None
        so = (C.c_int64 * 4)(*out.stride())
        mean, std, fill = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std), (C.c_uint8 * 3)(*self.fill)
        _lib.call("mgu_augment_affine_color", dev, images_u8, B, Hs, Ws, int(self.bgr), masks, self.num_classes, out, H, W, so, mean, std, fill,
                  mout, self.mask_fill, params, need_mean)
        return (out, mout) if masks is not None else out


ELASTIC_NODES = (4, 32)          # control nodes a side of mgu_augment_elastic_color
ELASTIC_CTRL_LIMIT = 1 << 26     # |c|, 16.16 source pixels


def bspline_weights_q14() -> np.ndarray:
    """The (256, 4) int32 weight table Wq of mgu_augment_elastic_color (include/mgunet.h, "elastic deformation"): the uniform cubic
    B-spline at t / 256 in Q14 from integers alone, every row summing to 16384 (the larger of w1, w2 takes the remainder, w1 on a tie).
    The library forms the same table itself."""
    T = 256
    D = 6 * T ** 3
    rows = []
    for t in range(T):
        n = ((T - t) ** 3, 3 * t ** 3 - 6 * T * t * t + 4 * T ** 3, -3 * t ** 3 + 3 * T * t * t + 3 * T * T * t + T ** 3, t ** 3)
        w = [(2 * 16384 * v + D) // (2 * D) for v in n]
        w[2 if w[2] > w[1] else 1] += 16384 - sum(w)
        rows.append(w)
    return np.asarray(rows, np.int32)


def elastic_control(normals, sigma: float, row, nodes) -> torch.Tensor:
    """The control nodes of one image for mgu_augment_elastic_color -> int32 (2, gh, gw) host tensor (plane 0 x, plane 1 y), 16.16
    SOURCE-pixel units.  normals: float64 (2, gh, gw) standard normal draws, each clipped to [-3, 3]; the vector in OUTPUT pixels is
    V = FIX16(sigma n), FIX16(v) = floor(v 65536 + 0.5).  It is carried into source units by the linear part a0, a1, a3, a4 of the image's
    table row in Python integers (no libm): cx = (a0 VX + a1 VY + 32768) >> 16, cy = (a3 VX + a4 VY + 32768) >> 16, so the warp turns
    and scales with the crop.  |c| > 2^26 raises."""
    gh, gw = int(nodes[0]), int(nodes[1])
    if not (ELASTIC_NODES[0] <= gh <= ELASTIC_NODES[1] and ELASTIC_NODES[0] <= gw <= ELASTIC_NODES[1]):
        raise ValueError(f"elastic_control: nodes {gh} x {gw} must be in [{ELASTIC_NODES[0]}, {ELASTIC_NODES[1]}] a side")
    n = np.asarray(normals, np.float64)
    if n.shape != (2, gh, gw) or not np.isfinite(n).all():
        raise ValueError(f"elastic_control: normals must be finite float64 (2, {gh}, {gw})")
    a0, a1, _a2, a3, a4 = (int(v) for v in row[:5])
    sg = float(sigma)
    vx = [_fix(sg * min(max(v, -3.0), 3.0), 16) for v in n[0].reshape(-1).tolist()]
    vy = [_fix(sg * min(max(v, -3.0), 3.0), 16) for v in n[1].reshape(-1).tolist()]
    cx = [(a0 * x + a1 * y + 32768) >> 16 for x, y in zip(vx, vy)]
    cy = [(a3 * x + a4 * y + 32768) >> 16 for x, y in zip(vx, vy)]
    if max(abs(v) for v in cx + cy) > ELASTIC_CTRL_LIMIT:
        raise ValueError(f"elastic_control: a control displacement beyond 2^26 (1024 source pixels): sigma {sg} is too large for this crop")
    return torch.tensor([cx, cy], dtype=torch.int32).reshape(2, gh, gw)


def elastic_field(ctrl: torch.Tensor, out_hw) -> torch.Tensor:
    """The displacement field of mgu_augment_elastic_color alone: ctrl int32 (B, 2, gh, gw) on the device -> int32 (B, 2, H, W), plane 0
    Dx, plane 1 Dy in 16.16 source pixels (mgu_elastic_field, one launch)."""
    if not isinstance(ctrl, torch.Tensor) or ctrl.dtype != torch.int32 or ctrl.dim() != 4 or ctrl.shape[1] != 2:
        raise TypeError("ctrl must be a (B, 2, gh, gw) int32 tensor")
    _lib.require_hip(ctrl, "mgunet.elastic_field")
    ctrl = ctrl.contiguous()
    B, _two, gh, gw = ctrl.shape
    H, W = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((B, 2, max(H, 0), max(W, 0)), device=ctrl.device, dtype=torch.int32)
    _lib.call("mgu_elastic_field", ctrl.device, ctrl, B, gh, gw, H, W, out)
    return out


class RandomElasticAffineColor(RandomAffineColor):
    """RandomAffineColor with a random elastic deformation folded into the same pass (Ronneberger et al. 2015, 3.1: displacement vectors on
    a coarse grid, sigma = 10 pixels, interpolated to every pixel), and an optional int32 instance map sampled with the same
    coordinates for Trainer.train_step(images, masks, instances=).  include/mgunet.h, mgu_augment_elastic_color: the displacement is one
    more term of the source coordinate, so the image is still resampled once and the launches are the parent's; integers only, bitwise
    equal to tests/augment_elastic_oracle.py.  nodes: (gh, gw) control nodes, 4..32 a side; sigma: standard deviation of a node's
    displacement in OUTPUT pixels (normals clipped to +-3); label_fill: the instance id outside the source (0: background).
    Draws, part of the interface: per image, in batch order, the parent's torch.rand(10, float64) and then -- sigma != 0 only --
    torch.randn(2 gh gw, float64) reshaped (2, gh, gw)."""

    def __init__(self, size, nodes=(6, 6), sigma=10.0, label_fill=0, **kw):
        super().__init__(size, **kw)
        self.nodes = (int(nodes[0]), int(nodes[1]))
        if not all(ELASTIC_NODES[0] <= v <= ELASTIC_NODES[1] for v in self.nodes):
            raise ValueError(f"nodes must be in [{ELASTIC_NODES[0]}, {ELASTIC_NODES[1]}] a side")
        self.sigma, self.label_fill = float(sigma), int(label_fill)
        if not (self.sigma >= 0.0 and math.isfinite(self.sigma)):
            raise ValueError("sigma must be non-negative")
        if not -2 ** 31 <= self.label_fill < 2 ** 31:
            raise ValueError("label_fill must fit int32")

    def draw(self, B: int, src_hw, generator=None):
        """-> (params (B, 16) int32, ctrl (B, 2, gh, gw) int32), host tensors; sigma == 0 draws no normals and gives zero nodes."""
        gh, gw = self.nodes
        rows, ctrl = [], []
        for _ in range(int(B)):
            rows.append(self.row(torch.rand(10, dtype=torch.float64, generator=generator).tolist(), src_hw))
            if self.sigma != 0.0:
                n = torch.randn(2 * gh * gw, dtype=torch.float64, generator=generator).reshape(2, gh, gw)
                ctrl.append(elastic_control(n.numpy(), self.sigma, rows[-1], self.nodes))
            else:
                ctrl.append(torch.zeros((2, gh, gw), dtype=torch.int32))
        return torch.tensor(rows, dtype=torch.int32).reshape(int(B), 16), torch.stack(ctrl).reshape(int(B), 2, gh, gw)

    def __call__(self, images_u8: torch.Tensor, masks: torch.Tensor = None, labels: torch.Tensor = None, generator=None,
                 out: torch.Tensor = None, params: torch.Tensor = None, ctrl: torch.Tensor = None):
        """images_u8, masks, out, params as RandomAffineColor; labels: optional (B, Hs, Ws) int32 instance map -> int32 (B, H, W).
        Returns the images and, in this order, whichever of masks and labels were given.  ctrl: explicit (B, 2, gh, gw) int32 nodes
        (any 4..32 a side).  With neither params nor ctrl both come from one draw; explicit params without ctrl are applied without a
        displacement.  sigma == 0 without ctrl and labels is the parent's call (mgu_augment_affine_color)."""
        if ctrl is None and labels is None and (self.sigma == 0.0 or params is not None):
            if params is None and isinstance(images_u8, torch.Tensor) and images_u8.dim() == 4:      # the parent's draws, not this class's pair
                params = RandomAffineColor.draw(self, images_u8.shape[0], images_u8.shape[1:3], generator)
            return super().__call__(images_u8, masks, generator=generator, out=out, params=params)
        if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
            raise TypeError("images_u8 must be a (B, Hs, Ws, 3) uint8 tensor")
        _lib.require_hip(images_u8, "mgunet.RandomElasticAffineColor")
        dev = images_u8.device
        images_u8 = images_u8.contiguous()
        B, Hs, Ws, _c = images_u8.shape
        H, W = self.size
        if masks is not None:
            if masks.dtype != torch.uint8 or masks.device != dev or tuple(masks.shape) != (B, Hs, Ws):
                raise ValueError("masks must be a (B, Hs, Ws) uint8 tensor on the images' device")
            masks = masks.contiguous()
        if labels is not None:
            if labels.dtype != torch.int32 or labels.device != dev or tuple(labels.shape) != (B, Hs, Ws):
                raise ValueError("labels must be a (B, Hs, Ws) int32 tensor on the images' device")
            labels = labels.contiguous()
        if out is None:
            out = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
        elif tuple(out.shape) != (B, 3, H, W) or out.dtype != torch.float32 or out.device != dev:
            raise ValueError("`out` must be a float32 (B, 3, H, W) tensor on the images' device")
        if params is None and ctrl is None:
            if self.sigma == 0.0:
                params = self.draw(B, (Hs, Ws), generator)[0]
            else:
                params, ctrl = self.draw(B, (Hs, Ws), generator)
        elif params is None:
            params = RandomAffineColor.draw(self, B, (Hs, Ws), generator)
        if tuple(params.shape) != (B, 16) or params.dtype != torch.int32:
            raise ValueError("params must be a (B, 16) int32 table")
        gh = gw = 0
        if ctrl is not None:
            if ctrl.dtype != torch.int32 or ctrl.dim() != 4 or tuple(ctrl.shape[:2]) != (B, 2):
                raise ValueError("ctrl must be a (B, 2, gh, gw) int32 tensor")
            gh, gw = int(ctrl.shape[2]), int(ctrl.shape[3])
            if not all(ELASTIC_NODES[0] <= v <= ELASTIC_NODES[1] for v in (gh, gw)):
                raise ValueError(f"ctrl: {gh} x {gw} control nodes, both must be in [{ELASTIC_NODES[0]}, {ELASTIC_NODES[1]}]")
            if not ctrl.is_cuda and ctrl.numel() and int(ctrl.abs().max()) > ELASTIC_CTRL_LIMIT:
                raise ValueError("ctrl: |c| must stay within 2^26")
            ctrl = ctrl.to(dev).contiguous()
        need_mean = 1 if params.is_cuda else int(bool((params[:, 15] != 0).any()))
        if not params.is_cuda and int(params[:, 6:].abs().max()) > COLOR_Q12_LIMIT:
            raise ValueError("params: |A| and |k| must stay within 2^15")
        params = params.to(dev).contiguous()
        mout = torch.empty((B, H, W), device=dev, dtype=torch.int64) if masks is not None else None
        lout = torch.empty((B, H, W), device=dev, dtype=torch.int32) if labels is not None else None
        so = (C.c_int64 * 4)(*out.stride())
        mean, std, fill = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std), (C.c_uint8 * 3)(*self.fill)
        _lib.call("mgu_augment_elastic_color", dev, images_u8, B, Hs, Ws, int(self.bgr), masks, self.num_classes, out, H, W, so, mean, std, fill,
                  mout, self.mask_fill, params, need_mean, labels, lout, self.label_fill, ctrl, gh, gw)
        res = [out] + [t for t in (mout, lout) if t is not None]
        return tuple(res) if len(res) > 1 else out


def _rgb_op(fn_name, image_array_rgb, out_channels):
    if isinstance(image_array_rgb, (np.ndarray, torch.Tensor)) and (image_array_rgb.ndim != 3 or image_array_rgb.shape[2] != 3):
        raise ValueError("Input image must be an RGB image (H, W, 3).")
    img, was_np = _to_dev_u8(image_array_rgb)
    H, W, _ = img.shape
    out = torch.empty((H, W, 3) if out_channels == 3 else (H, W), device=img.device, dtype=torch.uint8)
    _lib.call(fn_name, img.device, img, H, W, out)
    return out.cpu().numpy() if was_np else out


class EdgeDetector:
    def __init__(self, kernel_size=3):
        if kernel_size != 3:
            raise NotImplementedError("the HIP path implements the 3x3 Sobel operator (configs/preprocessing.yaml: sobel_kernel_size 3)")
        self.kernel_size = kernel_size

    def sobel_edges(self, image_array_rgb):
        """(H, W, 3) RGB uint8 -> (H, W) uint8 edge magnitude normalised to [0, 255]."""
        return _rgb_op("mgu_sobel_edges_u8", image_array_rgb, 1)


MAX_CLAHE_GRID = 64   # mgu_clahe_u8: tiles per axis


class CLAHE:
    """cv2.createCLAHE(clipLimit, tileGridSize) on uint8 as this build defines it (include/mgunet.h, mgu_clahe_u8): a clipped histogram and
    a byte table per tile, the four nearest tables blended bilinearly in fp32, every operation rounded on its own.  It follows OpenCV
    4.x's clahe.cpp for 8-bit images; cv2 is not a dependency, and equality with an actual cv2 build is not verified.  The defaults and
    the (x, y) order of tile_grid_size are cv2's; clip_limit <= 0 clips nothing.  A 3-channel image is equalised on the Y plane of cv2's
    YUV, as HistogramEqualizer.equalize_histogram_rgb."""

    def __init__(self, clip_limit=40.0, tile_grid_size=(8, 8)):
        self.clip_limit = float(clip_limit)
        if not math.isfinite(self.clip_limit):
            raise ValueError(f"clip_limit must be finite, got {clip_limit}")
        try:
            gx, gy = (int(v) for v in tile_grid_size)
        except (TypeError, ValueError):
            raise ValueError(f"tile_grid_size must be two integers (x, y), got {tile_grid_size!r}")
        if (gx, gy) != tuple(tile_grid_size) or not (1 <= gx <= MAX_CLAHE_GRID and 1 <= gy <= MAX_CLAHE_GRID):
            raise ValueError(f"tile_grid_size must be two integers in 1..{MAX_CLAHE_GRID} (x, y), got {tile_grid_size!r}")
        self.tile_grid_size = (gx, gy)

    @property
    def grid_yx(self):
        return self.tile_grid_size[1], self.tile_grid_size[0]

    @staticmethod
    def _batch_shape(images, channels):
        """(B, H, W, C) of what `images` holds, checked on the metadata alone"""
        if not isinstance(images, (np.ndarray, torch.Tensor)):
            raise TypeError("Input must be a NumPy array or a tensor.")
        if images.dtype != (np.uint8 if isinstance(images, np.ndarray) else torch.uint8):
            raise TypeError(f"expected a uint8 image, got {images.dtype}")
        s = tuple(int(v) for v in images.shape)
        if channels not in (None, 1, 3):
            raise ValueError(f"channels must be 1 or 3, got {channels}")
        if len(s) == 2 and channels in (None, 1):
            full = (1,) + s + (1,)
        elif len(s) == 3 and channels == 1 and s[2] != 1:
            full = s + (1,)                                  # a grey batch, only when stated
        elif len(s) == 3 and s[2] in (1, 3) and channels in (None, s[2]):
            full = (1,) + s
        elif len(s) == 4 and s[3] in (1, 3) and channels in (None, s[3]):
            full = s
        else:
            raise ValueError(f"expected (H, W), (H, W, 3), (B, H, W, 1 | 3) or, with channels=1, (B, H, W) uint8 images; got {s}"
                             + (f" with channels={channels}" if channels is not None else ""))
        if 0 in full:
            raise ValueError(f"expected non-empty images, got {s}")
        return full

    def _run(self, images, channels, out, tables):
        B, H, W, ch = self._batch_shape(images, channels)
        if out is not None and (type(out) is not type(images) or tuple(out.shape) != tuple(images.shape) or out.dtype != images.dtype):
            raise ValueError("`out` must be of the kind, shape and dtype of the images")
        img, was_np = _to_dev_u8(images)
        if out is None or was_np:
            res = torch.empty_like(img)
        else:
            if out.device != img.device or not out.is_contiguous():
                raise ValueError("`out` must be a contiguous tensor on the images' device")
            res = out
        gy, gx = self.grid_yx
        luts = torch.empty((B, gy, gx, 256), device=img.device, dtype=torch.uint8) if tables else None
        _lib.call("mgu_clahe_u8", img.device, img, B, H, W, ch, gy, gx, self.clip_limit, res, luts)
        if tables:
            return luts.cpu().numpy() if was_np else luts
        if not was_np:
            return res
        host = res.cpu().numpy()
        if out is None:
            return host
        out[...] = host
        return out

    def apply(self, images, out=None, channels=None):
        """(H, W), (H, W, 3), (B, H, W, 1 | 3) or -- only with channels=1 -- a (B, H, W) grey batch, uint8 -> the same shape, two launches
        for the batch.  numpy in -> numpy out, device tensor in -> device tensor out; out: where the result goes (the images themselves
        are allowed: in place)."""
        return self._run(images, channels, out, False)

    def tables(self, images, channels=None):
        """-> the uint8 (B, grid_y, grid_x, 256) tables of the tiles (B = 1 for one image)"""
        return self._run(images, channels, None, True)


class HistogramEqualizer:
    def equalize_histogram_rgb(self, image_array_rgb):
        """(H, W, 3) RGB uint8 -> (H, W, 3): luminance histogram equalised in YUV."""
        return _rgb_op("mgu_equalize_hist_rgb_u8", image_array_rgb, 3)

    def clahe_rgb(self, image_array_rgb, clip_limit=40.0, tile_grid_size=(8, 8)):
        """(H, W, 3) RGB uint8 -> (H, W, 3): CLAHE(clip_limit, tile_grid_size) on the luminance in YUV."""
        if isinstance(image_array_rgb, (np.ndarray, torch.Tensor)) and (image_array_rgb.ndim != 3 or image_array_rgb.shape[2] != 3):
            raise ValueError("Input image must be an RGB image (H, W, 3).")
        return CLAHE(clip_limit, tile_grid_size).apply(image_array_rgb, channels=3)

    def clahe_gray(self, image_array, clip_limit=40.0, tile_grid_size=(8, 8)):
        """(H, W) uint8 -> (H, W): CLAHE(clip_limit, tile_grid_size) of a grey image."""
        if isinstance(image_array, (np.ndarray, torch.Tensor)) and image_array.ndim != 2:
            raise ValueError("Input image must be a grey image (H, W).")
        return CLAHE(clip_limit, tile_grid_size).apply(image_array, channels=1)


MAX_GAUSSIAN_KSIZE = 31   # mgu_gaussian_blur_u8: the tile and its halo live in LDS

_SMALL_GAUSSIAN = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
                   7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}   # cv::getGaussianKernel for sigma <= 0


def gaussian_kernel_f64(ksize: int, sigma: float) -> np.ndarray:
    """The float64 weights of one axis as cv::getGaussianKernel defines them: for sigma <= 0 the fixed tables up to ksize 7, else
    sigma = 0.3 ((ksize - 1) 0.5 - 1) + 0.8; exp(-x^2 / (2 sigma^2)) at x = i - (ksize - 1) / 2, divided by the sum."""
    k = int(ksize)
    if k < 1 or k % 2 == 0:
        raise ValueError("Kernel size must be positive and odd.")
    s = float(sigma)
    if s <= 0 and k <= 7:
        return np.asarray(_SMALL_GAUSSIAN[k], np.float64)
    if s <= 0:
        s = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2
    w = np.exp(-(x * x) / (2.0 * s * s))
    return w / w.sum()


def gaussian_kernel_q8(ksize: int, sigma: float) -> np.ndarray:
    """The int32 Q8.8 weights of one axis that mgu_gaussian_blur_u8 takes: 256 gaussian_kernel_f64 rounded half to even from the
    outside in, each rounding error carried into the next tap, the centre tap taking what is left of 256.  Symmetric, non-negative,
    the sum exactly 256 (a constant image stays constant), every weight within 1 of 256 w.  (5, 1.0) -> [14, 62, 104, 62, 14]."""
    w = gaussian_kernel_f64(ksize, sigma)
    k = w.size
    q = np.zeros(k, np.int64)
    err = 0.0
    for i in range(k // 2):
        a = 256.0 * float(w[i]) + err
        q[i] = q[k - 1 - i] = int(np.rint(a))
        err = a - float(q[i])
    q[k // 2] = 256 - 2 * int(q[:k // 2].sum())
    return q.astype(np.int32)


class GaussianSmoother:
    """cv2.GaussianBlur on uint8 as this build defines it (include/mgunet.h, mgu_gaussian_blur_u8): separable Q8.8 integer weights,
    reflect-101 borders, integers only on the device.  It follows OpenCV 4.x's published fixed-point scheme for 8-bit images; cv2 is
    not a dependency, and equality with an actual cv2 build is not verified."""

    def __init__(self, kernel_size=(5, 5), sigma_x=1.0, sigma_y=None):
        self.kernel_size = kernel_size   # (width, height)
        self.sigma_x = sigma_x
        self.sigma_y = sigma_y if sigma_y is not None else sigma_x
        if not (self.kernel_size[0] > 0 and self.kernel_size[0] % 2 == 1 and self.kernel_size[1] > 0 and self.kernel_size[1] % 2 == 1):
            raise ValueError("Kernel size must be positive and odd.")
        if max(self.kernel_size[0], self.kernel_size[1]) > MAX_GAUSSIAN_KSIZE:
            raise NotImplementedError(f"the HIP path implements Gaussian kernels of up to {MAX_GAUSSIAN_KSIZE} x {MAX_GAUSSIAN_KSIZE} taps")

    def kernels(self):
        """-> (kx, ky) int32 Q8.8 weights; sigma_y <= 0 takes sigma_x, as cv2.GaussianBlur."""
        sx = float(self.sigma_x)
        sy = float(self.sigma_y) if self.sigma_y is not None else sx
        if sy <= 0:
            sy = sx
        return gaussian_kernel_q8(int(self.kernel_size[0]), sx), gaussian_kernel_q8(int(self.kernel_size[1]), sy)

    def _taps(self):
        kx, ky = self.kernels()
        return (C.c_int32 * kx.size)(*kx.tolist()), int(kx.size), (C.c_int32 * ky.size)(*ky.tolist()), int(ky.size)

    def smooth(self, image_array):
        """(H, W) or (H, W, C) uint8, C <= 4 -> the same shape; a (B, H, W, C) tensor is one launch.  numpy in -> numpy out, device
        tensor in -> device tensor out."""
        if (isinstance(image_array, np.ndarray) and image_array.dtype != np.uint8) or \
                (isinstance(image_array, torch.Tensor) and image_array.dtype != torch.uint8):
            raise NotImplementedError(f"the HIP path smooths uint8 images, got {image_array.dtype}")
        img, was_np = _to_dev_u8(image_array)
        if img.dim() not in (2, 3, 4) or (img.dim() >= 3 and not 1 <= img.shape[-1] <= 4) or img.numel() == 0:
            raise ValueError("expected a non-empty (H, W), (H, W, C) or (B, H, W, C) uint8 image with C <= 4")
        B = img.shape[0] if img.dim() == 4 else 1
        H, W = (img.shape[0], img.shape[1]) if img.dim() < 4 else (img.shape[1], img.shape[2])
        ch = 1 if img.dim() == 2 else img.shape[-1]
        out = torch.empty_like(img)
        _lib.call("mgu_gaussian_blur_u8", img.device, img, B, H, W, ch, *self._taps(), out)
        return out.cpu().numpy() if was_np else out


def _patch_column_args(images_u8, patch_size, per_channel, out, col0):
    """what the fused patch-column calls share: the (B, H, W, 3) device batch, the patch size, and the rows the columns go to (`out`
    checked, or a new (B*Np, 3 | 1) tensor at column 0)"""
    u8, _ = _to_dev_u8(images_u8)
    if u8.dim() == 3:
        u8 = u8.unsqueeze(0)
    if u8.dim() != 4 or u8.shape[3] != 3:
        raise ValueError("Input image must be an RGB image (H, W, 3) or a batch (B, H, W, 3).")
    B, H, W, _c = u8.shape
    p = int(patch_size)
    if p < 1:
        raise ValueError(f"patch_size must be positive, got {p}")
    rows, n = B * ((H + p - 1) // p) * ((W + p - 1) // p), 3 if per_channel else 1
    if out is None:
        out, col0 = torch.empty((rows, n), device=u8.device, dtype=torch.float32), 0
    elif out.dim() != 2 or out.shape[0] != rows or out.dtype != torch.float32 or out.device != u8.device or not out.is_contiguous():
        raise ValueError(f"`out` must be a contiguous float32 ({rows}, F) tensor on the images' device")
    return u8, p, out, int(col0)


def patch_smooth_features_u8(images_u8, patch_size: int, smoother: GaussianSmoother, per_channel: bool = False, out: torch.Tensor = None,
                             col0: int = 0) -> torch.Tensor:
    """patch_features_u8(smoother.smooth(image b), patch_size, per_channel) for every image of an (H, W, 3) / (B, H, W, 3) RGB uint8
    batch, bit for bit, in one launch and without the smoothed images: (B*Np, 3 | 1) float32, or columns [col0, col0 + (3 | 1)) of the
    contiguous float32 (B*Np, F) tensor `out`, whose other columns are left alone."""
    u8, p, out, col0 = _patch_column_args(images_u8, patch_size, per_channel, out, col0)
    B, H, W, _c = u8.shape
    _lib.call("mgu_patch_smooth_mean_u8", u8.device, u8, B, H, W, p, *smoother._taps(), 1 if per_channel else 0, out, out.shape[1], col0)
    return out


def patch_clahe_features_u8(images_u8, patch_size: int, clahe: CLAHE, per_channel: bool = False, out: torch.Tensor = None,
                            col0: int = 0) -> torch.Tensor:
    """patch_features_u8(clahe.apply(image b), patch_size, per_channel) for every image of an (H, W, 3) / (B, H, W, 3) RGB uint8 batch,
    bit for bit, in two launches and without the equalised images: (B*Np, 3 | 1) float32, or columns [col0, col0 + (3 | 1)) of the
    contiguous float32 (B*Np, F) tensor `out`, whose other columns are left alone."""
    if not isinstance(clahe, CLAHE):
        raise TypeError("clahe must be a CLAHE instance")
    u8, p, out, col0 = _patch_column_args(images_u8, patch_size, per_channel, out, col0)
    B, H, W, _c = u8.shape
    gy, gx = clahe.grid_yx
    _lib.call("mgu_patch_clahe_mean_u8", u8.device, u8, B, H, W, p, gy, gx, clahe.clip_limit, 1 if per_channel else 0, out, out.shape[1],
              col0)
    return out


def patch_features_u8(image, patch_size: int, per_channel: bool = False) -> torch.Tensor:
    """image_to_patches(map).mean(...) of scripts/graph_refinement.py:97-104 for a uint8 (H, W) / (H, W, C) map: per-patch means
    (zero padded bottom / right) -> (Np, 1) or (Np, C) float32 on the device."""
    img, _ = _to_dev_u8(image)
    if img.dim() == 2:
        img = img.unsqueeze(-1)
    H, W, ch = img.shape
    nph, npw = (H + patch_size - 1) // patch_size, (W + patch_size - 1) // patch_size
    out = torch.empty((nph * npw, ch if per_channel else 1), device=img.device, dtype=torch.float32)
    _lib.call("mgu_patch_mean_u8", img.device, img, H, W, ch, patch_size, 1 if per_channel else 0, out)
    return out


DEFAULT_COLORS_BGR = [(0, 0, 0), (0, 255, 0), (0, 0, 255), (255, 0, 0)]   # infer_segmentation.py:40-45


def postprocess_segmentation(seg_logits_or_probs, num_classes, colors=None):
    """infer_segmentation.py:20-51: (C, H, W) / (1, C, H, W) scores or (H, W) labels -> (labels (H, W) numpy, colour map (H, W, 3) uint8
    numpy).  Classes beyond the four fixed colours get random colours in the reference (np.random): pass `colors` to fix them."""
    t = seg_logits_or_probs
    _lib.require_hip(t, "mgunet.postprocess_segmentation")
    if t.ndim == 4:
        t = t.squeeze(0)
    if t.shape[0] == num_classes and t.ndim == 3:
        from .engine import argmax_classes
        labels = argmax_classes(t.unsqueeze(0).float())[0]
    else:
        labels = t.long()
    labels = labels.contiguous()
    pal = list(colors if colors is not None else DEFAULT_COLORS_BGR)
    if len(pal) < num_classes:
        raise ValueError(f"{num_classes} classes need {num_classes} colours (the reference draws the extra ones at random)")
    palette = torch.tensor(pal[:num_classes], dtype=torch.uint8, device=t.device).contiguous()
    H, W = labels.shape
    vis = torch.empty((H, W, 3), device=t.device, dtype=torch.uint8)
    _lib.call("mgu_colorize_labels", t.device, labels, H * W, palette, int(num_classes), vis, None)
    return labels.cpu().numpy(), vis.cpu().numpy()
