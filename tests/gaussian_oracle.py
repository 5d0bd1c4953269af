"""numpy form of the Gaussian blur the device computes (include/mgunet.h, mgu_gaussian_blur_u8), written from the definition and sharing
no code with the package.  Integers only after the weights are quantised.

    sigma       sigma_y None or <= 0 -> sigma_x; an axis with sigma <= 0: 0.3 ((k - 1) 0.5 - 1) + 0.8
    float w     sigma <= 0 and k <= 7: OpenCV's small tables; else exp(-x^2 / (2 sigma^2)), x = i - (k - 1) / 2, over the sum   (float64)
    Q8.8        i = 0 .. k//2 - 1: a = 256 w_i + err, q_i = q_{k-1-i} = rint(a) (half to even), err = a - q_i; centre = 256 - 2 sum q_i
    blur        h = sum_d kx[d] src[y][r(x + d - rx)];  v = sum_d ky[d] h[r(y + d - ry)][x];  out = (v + 32768) >> 16
    r           reflect-101 repeated until inside; n == 1 -> 0

This follows the fixed-point scheme OpenCV 4.x publishes for 8-bit GaussianBlur; it has not been compared with a cv2 build."""
import math

import numpy as np

SMALL = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16],
         7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def float_kernel(k, sigma):
    if sigma <= 0 and k <= 7:
        return np.array(SMALL[k], np.float64)
    if sigma <= 0:
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    w = np.array([math.exp(-((i - (k - 1) / 2) ** 2) / (2.0 * sigma * sigma)) for i in range(k)], np.float64)
    return w / w.sum()


def q8_kernel(k, sigma):
    w = float_kernel(k, sigma)
    q = [0] * k
    err = 0.0
    for i in range(k // 2):
        a = 256.0 * w[i] + err
        q[i] = q[k - 1 - i] = int(round(a))      # Python's round: half to even
        err = a - q[i]
    q[k // 2] = 256 - 2 * sum(q[:k // 2])
    return np.array(q, np.int64)


def kernels(kernel_size, sigma_x, sigma_y=None):
    """(kx, ky) of GaussianSmoother(kernel_size = (width, height), sigma_x, sigma_y)"""
    if sigma_y is None or sigma_y <= 0:
        sigma_y = sigma_x
    return q8_kernel(kernel_size[0], sigma_x), q8_kernel(kernel_size[1], sigma_y)


def reflect(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def taps_index(n, k):
    """(k, n) source index of tap d at position p"""
    return np.array([[reflect(p + d - k // 2, n) for p in range(n)] for d in range(k)], np.int64)


def pass_axis(a, q, axis):
    """sum_d q[d] * a[reflected index along axis] in int64"""
    idx = taps_index(a.shape[axis], len(q))
    out = np.zeros(a.shape, np.int64)
    for d in range(len(q)):
        out += int(q[d]) * np.take(a, idx[d], axis=axis)
    return out


def blur(img, kx, ky, vertical_first=False):
    """img: (H, W), (H, W, C) or (B, H, W, C) uint8 -> the same shape"""
    a = np.asarray(img)
    assert a.dtype == np.uint8
    ay, ax = (0, 1) if a.ndim < 4 else (1, 2)
    v = a.astype(np.int64)
    for q, axis in (((ky, ay), (kx, ax)) if vertical_first else ((kx, ax), (ky, ay))):
        v = pass_axis(v, q, axis)
    out = (v + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def smooth(img, kernel_size=(5, 5), sigma_x=1.0, sigma_y=None):
    kx, ky = kernels(kernel_size, sigma_x, sigma_y)
    return blur(img, kx, ky)


def patch_mean(img, patch, per_channel):
    """image_to_patches(map).mean(...) of an (H, W, C) uint8 map, zero padded bottom / right -> (Np, C | 1) float32, as mgu_patch_mean_u8"""
    H, W, C = img.shape
    nph, npw = -(-H // patch), -(-W // patch)
    pad = np.zeros((nph * patch, npw * patch, C), np.int64)
    pad[:H, :W] = img
    s = pad.reshape(nph, patch, npw, patch, C).sum((1, 3)).reshape(nph * npw, C)
    if per_channel:
        return (s.astype(np.float64) / (float(patch) * patch)).astype(np.float32)
    return (s.sum(1, keepdims=True).astype(np.float64) / (float(patch) * patch * C)).astype(np.float32)
