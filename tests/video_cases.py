"""Cases shared by the host tests (tests/test_video_host.py) and the GPU tests (tests/test_gpu_video.py) of the video stage.
Everything is generated from seeded numpy generators; nothing is read from disk."""
import numpy as np

TILE = 48      # mgu_frame_sad_tile() of the library these cases were written against (the GPU suite holds the two together)


def crops(seed, H, W, offsets, channels=3):
    """T frames (T, H, W[, 3]) cut from one noise image at `offsets` [(oy, ox), ...]: the true shift of pair (t, t+1) is
    offsets[t] - offsets[t+1], and the cost there is 0"""
    rng = np.random.default_rng(seed)
    oy, ox = max(o[0] for o in offsets), max(o[1] for o in offsets)
    big = rng.integers(0, 256, (oy + H, ox + W) + ((3,) if channels == 3 else ()), dtype=np.uint8)
    return np.stack([big[y:y + H, x:x + W] for y, x in offsets])


def true_shifts(offsets):
    o = np.asarray(offsets, np.int64)
    return (o[:-1] - o[1:]).astype(np.int32)


def _half_zero():
    f = crops(11, 44, 60, [(3, 1), (1, 4)], channels=1)
    f[:, :, :30] = 0                       # zero bytes on the reference side and on the searched side
    return f


def _zero_vs_255():
    f = np.zeros((2, 132, 136), np.uint8)
    f[1] = 255
    return f


# name -> (frames, radius, factor, bgr)
def registration_cases(tile=TILE):
    c = {
        "40x56 f1 R3": (crops(1, 40, 56, [(2, 3), (4, 1), (1, 0)]), 3, 1, False),
        "67x93 f2 R4": (crops(2, 67, 93, [(6, 0), (2, 4)]), 4, 2, False),
        "f8 smallest": (crops(3, 80, 80, [(8, 0), (0, 8)]), 1, 8, False),
        "f4 R2": (crops(4, 57, 70, [(4, 8), (0, 4), (8, 0)]), 2, 4, True),
        "T5 bgr": (crops(5, 36, 40, [(3, 3), (1, 4), (4, 0), (2, 2), (0, 3)]), 4, 1, True),
        "grey": (crops(6, 33, 47, [(0, 2), (3, 0)], channels=1), 3, 1, False),
        "uniform": (np.full((3, 30, 34, 3), 97, np.uint8), 4, 1, False),
        "uniform f2": (np.full((2, 60, 68), 13, np.uint8), 5, 2, False),
        "0 vs 255": (_zero_vs_255(), 2, 1, False),
        "half zero": (_half_zero(), 4, 1, False),
        "corner": (crops(7, 38, 42, [(0, 5), (5, 0)], channels=1), 5, 1, False),          # the minimum at (-R, +R)
        "corner f2": (crops(8, 76, 84, [(10, 0), (0, 10)]), 5, 2, False),                 # ... of the coarse square: (+5, -5) * 2
        "R32": (crops(9, 80, 76, [(30, 0), (0, 21)], channels=1), 32, 1, False),          # the largest radius
    }
    R = 2
    for k, (wh, ww) in enumerate([(tile - 1, 2 * tile + 1), (tile, 2 * tile), (tile + 1, 2 * tile - 1)]):
        c[f"tile {wh}x{ww}"] = (crops(20 + k, wh + 2 * R, ww + 2 * R, [(2, 0), (0, 1)], channels=1), R, 1, False)
    return c


# cases with a known answer: name -> (offsets, H, W, channels, radius, factor); every offset difference is a multiple of the factor
KNOWN = {
    "f1": ([(5, 2), (1, 6), (4, 0), (4, 0)], 40, 44, 3, 6, 1),
    "f2": ([(8, 2), (2, 6), (6, 0)], 64, 72, 1, 4, 2),
    "f4": ([(12, 0), (4, 8), (8, 4)], 96, 100, 3, 3, 4),
}


# ---- the track scene -----------------------------------------------------------------------------------------------------------------
# A static world of discs (cy, cx, radius, class) seen by a camera that walks right and wobbles up and down: discs enter on the right
# and leave on the left; two discs of different classes touch; disc 5 is half visible in frame 2; of disc 6 one pixel shows in frame 3
# and the whole in frame 4 (its track survives only when the link uses visible areas).
DISCS = [(20, 20, 7, 1), (40, 34, 6, 2), (24, 70, 6, 1), (24, 82, 6, 2), (18, 120, 6, 2), (44, 86, 6, 2), (30, 100, 7, 1), (40, 140, 7, 1)]
CAMERA = [(8, 0), (6, 10), (9, 22), (7, 30), (8, 44), (10, 52)]       # (oy, ox) of the six frames
TRACK_HW = (48, 64)
TRACK_RADIUS = 16
WORLD_HW = (64, 160)


def track_scene():
    """-> frames uint8 (6, 48, 64, 3), class map int64 (6, 48, 64), disc map int64 (6, 48, 64) (disc index + 1, 0 = none), the true
    shifts int32 (5, 2)"""
    rng = np.random.default_rng(42)
    H, W = TRACK_HW
    world = rng.integers(0, 256, WORLD_HW + (3,), dtype=np.uint8)
    cls, disc = np.zeros(WORLD_HW, np.int64), np.zeros(WORLD_HW, np.int64)
    yy, xx = np.mgrid[:WORLD_HW[0], :WORLD_HW[1]]
    for k, (cy, cx, r, c) in enumerate(DISCS):
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        cls[m], disc[m] = c, k + 1
    cut = lambda a: np.stack([a[y:y + H, x:x + W] for y, x in CAMERA])  # noqa: E731
    return cut(world), cut(cls), cut(disc), true_shifts(CAMERA)
