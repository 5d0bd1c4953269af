"""numpy restatements for mgunet.patch_inputs (no GPU, no torch): the per-patch label vote and the float64 patch pixel mean."""
import numpy as np


def patch_grid(H, W, p):
    return -(-H // p), -(-W // p)


def patch_label_vote(label_map, p, C):
    """(H, W) integer map -> (labels (Np,) int64, counts (Np, C) int32, purity (Np,) float32), patches in raster order.  Per patch:
    bincount over its real pixels (pad pixels do not exist here; values outside [0, C) are dropped), first maximum (np.argmax: the
    lowest class on ties), purity = float32(float64 count / float64 real pixels); no counted pixel: label 0, purity 0."""
    m = np.asarray(label_map).astype(np.int64)
    H, W = m.shape
    nph, npw = patch_grid(H, W, p)
    labels = np.zeros(nph * npw, np.int64)
    counts = np.zeros((nph * npw, C), np.int32)
    purity = np.zeros(nph * npw, np.float32)
    for py in range(nph):
        for px in range(npw):
            v = m[py * p:(py + 1) * p, px * p:(px + 1) * p].reshape(-1)     # slicing clips at the image: real pixels only
            k = py * npw + px
            counts[k] = np.bincount(v[(v >= 0) & (v < C)], minlength=C)[:C]
            best = int(np.argmax(counts[k]))
            if counts[k, best] > 0:
                labels[k] = best
                purity[k] = np.float32(np.float64(counts[k, best]) / np.float64(v.size))
    return labels, counts, purity


def patch_pixel_mean(image_chw, p):
    """(3, H, W) float image -> (Np,) float64: patches.mean(dim=[1,2,3]) of the zero-padded image (divisor 3 p^2), in float64."""
    x = np.asarray(image_chw, np.float64)
    Cc, H, W = x.shape
    nph, npw = patch_grid(H, W, p)
    pad = np.zeros((Cc, nph * p, npw * p), np.float64)
    pad[:, :H, :W] = x
    return pad.reshape(Cc, nph, p, npw, p).sum(axis=(0, 2, 4)).reshape(-1) / (Cc * p * p)
