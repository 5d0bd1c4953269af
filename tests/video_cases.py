"""Cases shared by the host tests (tests/test_video_host.py) and the GPU tests (tests/test_gpu_video.py, test_gpu_video_paths.py) of the video stage.
Everything is generated from seeded numpy generators; nothing is read from disk."""
import numpy as np

TILE = 48      # mgu_frame_sad_tile() of the library these cases were written against (the GPU suite holds the two together)
THREADS = 256  # lanes of a frame_sad_kernel workgroup


# ---- a mirror of frame_sad_kernel's work split (csrc/video.hip: sad_chunk and the kernel's th / tw / nsy / S) -------------------------------
# It says which shape reaches which path of the kernel; a change to the kernel's split must change it too, as TILE follows
# mgu_frame_sad_tile().  tests/test_video_host.py holds the case tables against it.
def sad_split(r):
    """(D, G, CH): y- or x-shifts of a level of radius r, groups of four x-offsets, y-shifts per workgroup (CH < D: grid.z chunks)"""
    D, G = 2 * r + 1, (2 * r + 7) // 4
    return D, G, D if D * G <= THREADS else THREADS // G


def sad_workgroups(Hp, Wp, M, r, tile=TILE):
    """the distinct (th, tw, nsy, S) of the workgroups a level launches on planes Hp x Wp with margin M at radius r: tile height and
    width, y-shifts of the chunk, row slices per task"""
    D, G, CH = sad_split(r)
    wh, ww = Hp - 2 * M, Wp - 2 * M
    edge = lambda n: {min(tile, n - k) for k in range(0, n, tile)}  # noqa: E731
    out = set()
    for th in edge(wh):
        for tw in edge(ww):
            for nsy in {min(CH, D - lo) for lo in range(0, D, CH)}:
                out.add((th, tw, nsy, max(1, min(th, THREADS // (nsy * G)))))
    return out


def sad_paths(Hp, Wp, M, r, min_th=1, tile=TILE):
    """the (row path, chunked?, S > 1?, tail) combinations a level launches: 'whole' = the from-registers path of a tile `tile` wide
    (tail 0), 'word' = the word-by-word path with a masked tail of tw % 4 bytes.  min_th: only tiles at least that high."""
    D, _, CH = sad_split(r)
    return {("whole" if tw == tile else "word", CH < D, S > 1, 0 if tw == tile else tw & 3)
            for th, tw, nsy, S in sad_workgroups(Hp, Wp, M, r, tile) if th >= min_th}


def levels(H, W, R, f):
    """(Hp, Wp, M, r) of the levels frame_shifts searches on H x W frames: the coarse one, and the fine one when f > 1"""
    return [(H // f, W // f, R, R)] + ([(H, W, f * R + f, f)] if f > 1 else [])


def case_paths(frames, R, f, min_th=1):
    return set().union(*(sad_paths(*lv, min_th=min_th) for lv in levels(frames.shape[1], frames.shape[2], R, f)))


def offsets_for(shifts):
    """crop offsets [(oy, ox), ...] whose true_shifts are `shifts`, the smallest non-negative ones"""
    o = np.concatenate([np.zeros((1, 2), np.int64), -np.cumsum(np.asarray(shifts, np.int64), axis=0)])
    return [tuple(int(v) for v in row) for row in o - o.min(axis=0)]


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


# ---- cases for every work split of frame_sad_kernel (too big for brute_surface's Python triple loop) ---------------------------------------
# name -> (H, W, R, true shifts); grey, factor 1, cut with crops() so that every pair's cost at its true shift is 0.  With sad_split's
# chunks the y-index sy + R of the shifts lies in the first chunk, in the short last one and on both sides of a chunk boundary, and
# sx reaches -R and +R.
PATH_SHAPES = {
    # whole-row, unchunked, S = 1 (th = 48); word path with tail 3
    "R13": (74, 121, 13, [(-13, 13), (13, -13), (0, 5), (4, -2)]),
    # whole-row, chunked: the full chunk (28 y-shifts) S = 1, the last (3) S > 1; bottom tiles th = 1; word path with tail 1
    "R15": (79, 127, 15, [(-15, 15), (12, -15), (13, 4), (15, -2)]),
    # window 50 x 48: a second tile row of height 2 under chunking
    "R15 tall": (80, 78, 15, [(15, -15), (13, 15), (12, -6), (-15, 1)]),
    # window 48 x 96: two full tiles, chunks of 28 + 5
    "R16": (80, 128, 16, [(-16, 16), (11, -16), (12, 5), (16, -3)]),
    # the largest radius on the whole-row path: chunks of 15, 15, 15, 15, 5; word path with tail 1
    "R32": (112, 113, 32, [(30, -21), (-32, 11), (17, 0), (-17, -32), (-18, 32)]),
}


def path_cases():
    """name -> (frames, radius, factor, bgr) like registration_cases(); true_shifts(path_offsets(name)) are the answers"""
    return {n: (crops(40 + k, H, W, offsets_for(s), channels=1), R, 1, False) for k, (n, (H, W, R, s)) in enumerate(PATH_SHAPES.items())}


def path_offsets(name):
    return offsets_for(PATH_SHAPES[name][3])


# ---- contents that a subtly wrong kernel gets wrong ---------------------------------------------------------------------------------------
CARRY = (4200, 4100, 1)                    # H, W, R of the all-0 against all-255 pair: every cost is 255 * 4198 * 4098 > 2^32
CARRY_COST = 255 * 4198 * 4098

TIE_HW, TIE_RADIUS = (50, 58), 9           # 19 * 19 = 361 surface entries: more than the pick's 256 threads
TIE_SHIFTS = {(2, 2): (-1, -1), (2, 3): (-1, 1), (3, 2): (1, -1), (1, 4): (0, 1), (4, 1): (1, 0)}   # period -> the definition's choice


def tie_frames(period):
    """two frames tiled with a py x px block of distinct bytes, the second moved by (1, 1): every shift = (1, 1) modulo the period
    costs 0, so sy^2 + sx^2, then sy, then sx decide"""
    py, px = period
    H, W = TIE_HW
    block = np.random.default_rng(70 + 10 * py + px).permutation(256)[:py * px].astype(np.uint8).reshape(py, px)
    yy, xx = np.mgrid[:H, :W]
    return np.stack([block[yy % py, xx % px], block[(yy - 1) % py, (xx - 1) % px]])


def low_amplitude_cases():
    """bytes from {0, 1} or {254, 255}: every coarse pixel sits on a rounding edge.  H, W = 26 f + f - 1, 25 f + f - 1: as many trailing
    rows and columns as can be dropped, Wc = 25 is no multiple of 4.  name -> (frames, radius, factor, bgr)"""
    c = {}
    for k, f in enumerate((2, 4, 8)):
        H, W = 26 * f + f - 1, 25 * f + f - 1
        for j, base in enumerate((0, 254)):
            rng = np.random.default_rng(80 + 2 * k + j)
            c[f"{base}+ f{f}"] = ((base + rng.integers(0, 2, (3, H, W))).astype(np.uint8), 2, f, False)
        if f == 8:
            c["254+ f8 bgr"] = ((254 + np.random.default_rng(90).integers(0, 2, (3, H, W, 3))).astype(np.uint8), 2, f, True)
    return c


def alternating_columns():
    """columns 0 / 255 at radius 15 on R15's shape: every per-lane sum is 0 or the tile's maximum; frame 2 starts on the other column"""
    H, W, R, _ = PATH_SHAPES["R15"]
    f = np.zeros((3, H, W), np.uint8)
    f[:2, :, 1::2] = 255
    f[2, :, 0::2] = 255
    return f, R, 1, False


# ---- label maps for track_align, link_objects and VideoCounter ------------------------------------------------------------------------------
def blob_maps(seed, T, H, W, n, classes=2, size=(2, 7)):
    """class maps int64 (T, H, W): n random rectangles a frame, sides in [size[0], size[1]), classes 1..classes"""
    rng = np.random.default_rng(seed)
    m = np.zeros((T, H, W), np.int64)
    for t in range(T):
        for _ in range(n):
            h, w = rng.integers(size[0], size[1], 2)
            y, x = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
            m[t, y:y + h, x:x + w] = rng.integers(1, classes + 1)
    return m


ALIGN_HW = (40, 52)
ALIGN_SHIFTS = [(0, 0), (3, -4), (-3, 4), (39, 0), (0, -51), (40, 0), (0, 52), (-2**31 + 1, 2**31 - 1)]   # one-line and empty rectangles


def align_maps():
    """class maps (8, 40, 52): random rectangles, and objects along all four edges, so a one-line common rectangle is not empty"""
    m = blob_maps(60, 8, *ALIGN_HW, 14)
    m[:, 0, :], m[:, -1, :], m[:, 2:-2, 0], m[:, 2:-2, -1] = 1, 2, 2, 1
    return m


def checkerboard_maps():
    """(3, 13, 19): two 4-connected checkerboards of two classes (every pixel its own object: every lane of a wave holds another key)
    around one frame-filling object; 13 * 19 = 247 is no multiple of 64"""
    yy, xx = np.mgrid[:13, :19]
    m = np.stack([1 + (yy + xx) % 2, np.ones_like(yy), 2 - (yy + xx) % 2]).astype(np.int64)
    return m, np.array([[1, -2], [0, 3]], np.int32)


# ---- track_ids with many objects ------------------------------------------------------------------------------------------------------------
MANY_COUNTS = [700, 0, 256, 257, 1, 513]


def many_links(older_frames=(2, 4), seed=7):
    """offsets int64 (7), link int64 (N), class_id int64 (N).  In a frame t of older_frames one object in eight links to a distinct
    object of frame t - 2 that no object of frame t - 1 continues; every other object links with probability 1/2 to a distinct object
    of frame t - 1 (as long as there are any); the rest are -1.  older_frames says where a video may NOT be cut into calls: a call
    that starts at frame t - 1 cannot carry a link into frame t - 2."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(MANY_COUNTS)]).astype(np.int64)
    N = int(off[-1])
    link = np.full(N, -1, np.int64)
    for t in range(1, len(MANY_COUNTS)):
        mine = rng.permutation(np.arange(off[t], off[t + 1]))
        if t in older_frames:
            older = np.arange(off[t - 2], off[t - 1])
            older = rng.permutation(older[~np.isin(older, link[off[t - 1]:off[t]])])
            k = min(mine.size // 8 + 1, older.size)
            link[mine[:k]], mine = older[:k], mine[k:]
        before = rng.permutation(np.arange(off[t - 1], off[t]))
        want = mine[rng.random(mine.size) < 0.5]
        k = min(want.size, before.size)
        link[want[:k]] = before[:k]
    return off, link, rng.integers(1, 3, N).astype(np.int64)


def cut_links(off, link, cls, lo, hi):
    """frames lo..hi (inclusive) of a link table as a table of their own: offsets from 0, links rebased (frame lo's become -1: its
    ids are carried), classes"""
    o0, o1 = int(off[lo]), int(off[hi + 1])
    l = link[o0:o1] - o0
    assert (l[int(off[lo + 1]) - o0:][link[int(off[lo + 1]):o1] >= 0] >= 0).all(), "a link crosses the cut"
    return off[lo:hi + 2] - o0, np.where(l >= 0, l, -1), cls[o0:o1]


# ---- a dense world: about 300 objects a frame -----------------------------------------------------------------------------------------------
DENSE_HW, DENSE_CAMERA, DENSE_RADIUS = (96, 128), [(4, 0), (0, 5), (7, 9)], 8


def dense_scene(seed=5):
    """-> frames uint8 (3, 96, 128, 3), class maps int64 (3, 96, 128), true shifts int32 (2, 2): jittered 2-4 px rectangles of two
    classes, one per cell of a 6-px grid, over a noise world seen from three camera positions"""
    rng = np.random.default_rng(seed)
    H, W = DENSE_HW
    wh, ww = H + max(c[0] for c in DENSE_CAMERA), W + max(c[1] for c in DENSE_CAMERA)
    world = rng.integers(0, 256, (wh, ww, 3), dtype=np.uint8)
    cls = np.zeros((wh, ww), np.int64)
    for gy in range(0, wh - 5, 6):
        for gx in range(0, ww - 5, 6):
            h, w = rng.integers(2, 5, 2)
            y, x = gy + rng.integers(0, 7 - h), gx + rng.integers(0, 7 - w)
            cls[y:y + h, x:x + w] = rng.integers(1, 3)
    cut = lambda a: np.stack([a[y:y + H, x:x + W] for y, x in DENSE_CAMERA])  # noqa: E731
    return cut(world), cut(cls), true_shifts(DENSE_CAMERA)
