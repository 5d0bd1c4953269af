"""numpy / scipy oracle of mgunet.clean_masks, shared by the cleanup tests.  It follows the definition of include/mgunet.h
(mgu_clean_masks) stage by stage, with scipy structuring elements instead of pixel loops:
  0. classes 1 .. num_classes - 1 are foreground; every other value reads as background (0).
  1. close: per class c, on the plane padded with background, Dil = A_c (+) D and Clo = {p : p + D inside Dil}; a background pixel
     takes the smallest c with p in Clo.
  2. fill: the 4-connected components of the background that touch no border, are no larger than max_hole_area (when > 0) and whose
     foreground 4-neighbours hold one class c become c.
  3. open: per class c, E = the pixels of A_c with no image pixel of another value within the disc (outside the image does not erode);
     a pixel of A_c stays iff a pixel of E lies within the disc.
D(r2) = {d : |d|^2 <= r2}.  Every function takes one (H, W) image; clean() takes a batch."""
import numpy as np
from scipy import ndimage

CROSS = ndimage.generate_binary_structure(2, 1)


def radius_sq(radius) -> int:
    """floor(radius^2), as mgunet.clean_masks squares its radii"""
    return int(np.floor(float(radius) ** 2 + 1e-9))


def disc(r2):
    """bool (2r + 1, 2r + 1): the structuring element D(r2)"""
    r = int(np.floor(np.sqrt(r2)))
    while (r + 1) ** 2 <= r2:
        r += 1
    while r * r > r2:
        r -= 1
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return y * y + x * x <= r2


def normalise(m, num_classes):
    m = np.asarray(m).astype(np.int64)
    return np.where((m >= 1) & (m < num_classes), m, 0)


def close(m, num_classes, r2):
    m = normalise(m, num_classes)
    if r2 <= 0:
        return m
    se = disc(r2)
    r = se.shape[0] // 2
    out = m.copy()
    for c in range(num_classes - 1, 0, -1):   # descending: the smallest class is written last
        a = np.pad(m == c, 2 * r)
        clo = ndimage.binary_erosion(ndimage.binary_dilation(a, se), se)[2 * r:-2 * r, 2 * r:-2 * r]
        out[clo & (m == 0)] = c
    return out


def fill(m, num_classes, max_hole_area=0):
    m = normalise(m, num_classes)
    out = m.copy()
    lab, n = ndimage.label(m == 0, CROSS)
    if n == 0:
        return out
    border = np.zeros(n + 1, bool)
    for edge in (lab[0], lab[-1], lab[:, 0], lab[:, -1]):
        border[edge] = True
    area = np.bincount(lab.ravel(), minlength=n + 1)
    lo, hi = np.full(n + 1, 1 << 30), np.zeros(n + 1, np.int64)   # min and max class among the foreground 4-neighbours
    H, W = m.shape
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        p = lab[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]     # the background pixel ...
        q = m[max(0, dy):H - max(0, -dy), max(0, dx):W - max(0, -dx)]       # ... and its neighbour at (dy, dx)
        sel = (p > 0) & (q > 0)
        np.minimum.at(lo, p[sel], q[sel])
        np.maximum.at(hi, p[sel], q[sel])
    hole = ~border & (lo == hi)
    if max_hole_area > 0:
        hole &= area <= max_hole_area
    hole[0] = False
    out[hole[lab]] = lo[lab][hole[lab]]
    return out


def open_(m, num_classes, r2):
    m = normalise(m, num_classes)
    if r2 <= 0:
        return m
    se = disc(r2)
    out = m.copy()
    for c in range(1, num_classes):
        a = m == c
        e = ndimage.binary_erosion(a, se, border_value=1)
        out[a & ~ndimage.binary_dilation(e, se)] = 0
    return out


def clean(maps, num_classes, close_r2=0, fill_holes=True, max_hole_area=0, open_r2=0):
    """(int64 (B, H, W) result, int64 (B, 3) [gained by closing, filled, removed by opening]) of a batch of class maps"""
    maps = np.asarray(maps)
    out, counts = np.zeros(maps.shape, np.int64), np.zeros((maps.shape[0], 3), np.int64)
    for b, m in enumerate(maps):
        m0 = normalise(m, num_classes)
        m1 = close(m0, num_classes, close_r2)
        m2 = fill(m1, num_classes, max_hole_area) if fill_holes else m1
        m3 = open_(m2, num_classes, open_r2)
        out[b] = m3
        counts[b] = [(m1 != m0).sum(), (m2 != m1).sum(), (m3 != m2).sum()]
    return out, counts


def argmax_first(logits_nchw):
    """first maximal class of (B, C, H, W) logits"""
    return np.argmax(np.asarray(logits_nchw), axis=1).astype(np.int64)


# ---- scenes shared by the host and the device tests -----------------------------------------------------------------------------
def disc_mask(shape, cy, cx, R):
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    return (y - cy) ** 2 + (x - cx) ** 2 <= R * R


PIN_HOLES = [((), 1), (((32, 32),), 1), (((32, 26),), 1), (((26, 26), (38, 38)), 2), (((32, 22), (32, 42)), 2),
             (((24, 32), (40, 32), (32, 24)), 3)]   # (pin holes (y, x), objects split_objects finds without hole filling)


def pin_hole_scene(holes):
    m = disc_mask((64, 64), 32, 32, 20).astype(np.int64)
    for y, x in holes:
        m[y, x] = 0
    return m


def bar_scene():
    """two discs of R = 9 joined by a bar of two rows: one component, two after opening with r2 = 1"""
    m = disc_mask((40, 72), 20, 18, 9) | disc_mask((40, 72), 20, 52, 9)
    m[20:22, 18:52] = True
    return m.astype(np.int64)


def crack_scene():
    """a disc of R = 12 cut by a zeroed column: two components, one after closing with r2 = 1"""
    m = disc_mask((40, 40), 20, 20, 12).astype(np.int64)
    m[:, 20] = 0
    return m


def chain_scene():
    """a 6 x 6 image whose border ring is background and whose inside is foreground but for the diagonal (1,1), (2,2), (3,3): the
    three are separate 4-connected components; (1,1) joins the border ring through (0,1), the other two are holes"""
    m = np.zeros((6, 6), np.int64)
    m[1:5, 1:5] = 1
    for k in (1, 2, 3):
        m[k, k] = 0
    return m
