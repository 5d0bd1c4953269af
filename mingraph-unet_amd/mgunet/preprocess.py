"""Host-side mirrors of the reference's input / output pipeline, routed through libmgunet.so:

    ImagePreprocessor        preprocessing/image_preprocessing/image_preprocess.py:6-126
    EdgeDetector             preprocessing/graph_feature_processing/edge_detection.py:4-44
    HistogramEqualizer       preprocessing/graph_feature_processing/histogram_equalization.py:4-49
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
augments only the image), and RandomFlipRotate augments a whole device batch in one launch."""
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


class HistogramEqualizer:
    def equalize_histogram_rgb(self, image_array_rgb):
        """(H, W, 3) RGB uint8 -> (H, W, 3): luminance histogram equalised in YUV."""
        return _rgb_op("mgu_equalize_hist_rgb_u8", image_array_rgb, 3)


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


def patch_smooth_features_u8(images_u8, patch_size: int, smoother: GaussianSmoother, per_channel: bool = False, out: torch.Tensor = None,
                             col0: int = 0) -> torch.Tensor:
    """patch_features_u8(smoother.smooth(image b), patch_size, per_channel) for every image of an (H, W, 3) / (B, H, W, 3) RGB uint8
    batch, bit for bit, in one launch and without the smoothed images: (B*Np, 3 | 1) float32, or columns [col0, col0 + (3 | 1)) of the
    contiguous float32 (B*Np, F) tensor `out`, whose other columns are left alone."""
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
    _lib.call("mgu_patch_smooth_mean_u8", u8.device, u8, B, H, W, p, *smoother._taps(), 1 if per_channel else 0, out, out.shape[1], int(col0))
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
