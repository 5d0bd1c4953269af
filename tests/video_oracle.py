"""numpy oracle of the video stage (csrc/video.hip, mgunet/video.py): frame registration by exhaustive byte-SAD search, the pair
alignment of label maps, links on visible areas and track ids.  This build's own definition (include/mgunet.h, "video"); integers
only, so every comparison against it is exact.  `variant` switches in one deliberate mistake at a time: the host tests show that each
differs from the definition on a shared case."""
import numpy as np

FACTORS = (1, 2, 4, 8)


def luma(frames: np.ndarray, bgr: bool = False) -> np.ndarray:
    """uint8 (T, H, W): (77 R + 150 G + 29 B + 128) >> 8; a grey (T, H, W) input is its own luma"""
    f = np.asarray(frames)
    assert f.dtype == np.uint8
    if f.ndim == 3:
        return f.copy()
    c = f.astype(np.int64)
    if bgr:
        c = c[..., ::-1]
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def coarse(y: np.ndarray, f: int) -> np.ndarray:
    """(T, H // f, W // f) uint8: rounded means of the f x f blocks, trailing rows and columns dropped"""
    T, H, W = y.shape
    Hc, Wc = H // f, W // f
    s = y[:, :Hc * f, :Wc * f].astype(np.int64).reshape(T, Hc, f, Wc, f).sum(axis=(2, 4))
    return ((s + f * f // 2) // (f * f)).astype(np.uint8)


def surface(A: np.ndarray, B: np.ndarray, M: int, r: int, centre=(0, 0), variant=None) -> np.ndarray:
    """int64 (2r+1, 2r+1): cost[sy + r][sx + r] = sum over p in [M, H-M) x [M, W-M) of |A(p) - B(p + centre + s)|"""
    H, W = A.shape
    a, b = A.astype(np.int64), B.astype(np.int64)
    out = np.zeros((2 * r + 1, 2 * r + 1), np.int64)
    for sy in range(-r, r + 1):
        for sx in range(-r, r + 1):
            ty, tx = centre[0] + sy, centre[1] + sx
            if variant == "sign":
                ty, tx = -ty, -tx
            y0, y1, x0, x1 = M, H - M, M, W - M
            if variant == "shrunk":        # the window of the pixels whose partner lies inside the plane: another one per shift
                y0, y1, x0, x1 = max(0, -ty), min(H, H - ty), max(0, -tx), min(W, W - tx)
            wa, wb = a[y0:y1, x0:x1], b[y0 + ty:y1 + ty, x0 + tx:x1 + tx]
            d = np.abs(wa - wb)
            if variant == "masked":        # a masked SAD skips the reference bytes that are 0
                d = d * (wa != 0)
            out[sy + r, sx + r] = d.sum()
    return out


def pick(surf: np.ndarray, variant=None):
    """(sy, sx) of the smallest cost; ties: the smallest sy^2 + sx^2, then the smaller sy, then the smaller sx"""
    r = surf.shape[0] // 2
    if variant == "first":                 # the first minimum in raster order
        i = int(np.argmin(surf))
        return i // surf.shape[1] - r, i % surf.shape[1] - r
    best = None
    for sy in range(-r, r + 1):
        for sx in range(-r, r + 1):
            key = (int(surf[sy + r, sx + r]), sy * sy + sx * sx, sy, sx)
            if variant == "last":          # the nearest minimum, but the last of several in raster order
                key = key[:2] + (-sy, -sx)
            if best is None or key < best[0]:
                best = (key, sy, sx)
    return best[1], best[2]


def frame_shifts(frames, radius: int, factor: int = 1, bgr: bool = False, variant=None):
    """-> shifts int32 (T-1, 2), cost int64 (T-1, 2), coarse surface int64 (T-1, 2R+1, 2R+1)"""
    y = luma(frames, bgr)
    T, H, W = y.shape
    R, f = int(radius), int(factor)
    assert T >= 2 and 1 <= R <= 32 and f in FACTORS
    c = coarse(y, f)
    Hc, Wc = c.shape[1:]
    if Hc - 2 * R < 8 or Wc - 2 * R < 8:
        raise ValueError("window under 8 x 8")
    shifts, cost, surfs = np.zeros((T - 1, 2), np.int32), np.zeros((T - 1, 2), np.int64), np.zeros((T - 1, 2 * R + 1, 2 * R + 1), np.int64)
    for t in range(T - 1):
        sc = surface(c[t], c[t + 1], R, R, variant=variant)
        surfs[t] = sc
        sy, sx = pick(sc, variant)
        if f == 1:
            shifts[t], cost[t] = (sy, sx), (sc[sy + R, sx + R], sc[R, R])
        else:
            sf = surface(y[t], y[t + 1], f * R + f, f, (f * sy, f * sx), variant=variant)
            dy, dx = pick(sf, variant)
            shifts[t], cost[t] = (f * sy + dy, f * sx + dx), (sf[dy + f, dx + f], sf[f, f])
    return shifts, cost, surfs


def brute_surface(A, B, R):
    """the coarse surface by the definition's triple loop (tiny planes only)"""
    H, W = A.shape
    out = np.zeros((2 * R + 1, 2 * R + 1), np.int64)
    for sy in range(-R, R + 1):
        for sx in range(-R, R + 1):
            s = 0
            for py in range(R, H - R):
                for px in range(R, W - R):
                    s += abs(int(A[py, px]) - int(B[py + sy, px + sx]))
            out[sy + R, sx + R] = s
    return out


# ---- labels --------------------------------------------------------------------------------------------------------------------------
def label_frames(classmap: np.ndarray):
    """8-connected components of equal non-zero class per frame, numbered in raster order of their first pixel (what
    mgunet.connected_components writes): labels int32 (T, H, W), offsets int64 (T+1), class_id int64 (N), area int64 (N)"""
    T, H, W = classmap.shape
    labels = np.zeros((T, H, W), np.int32)
    offsets, cls, area = [0], [], []
    for t in range(T):
        n = 0
        for y in range(H):
            for x in range(W):
                if classmap[t, y, x] == 0 or labels[t, y, x]:
                    continue
                n += 1
                v, stack, a = classmap[t, y, x], [(y, x)], 0
                labels[t, y, x] = n
                while stack:
                    cy, cx = stack.pop()
                    a += 1
                    for ny in range(max(cy - 1, 0), min(cy + 2, H)):
                        for nx in range(max(cx - 1, 0), min(cx + 2, W)):
                            if classmap[t, ny, nx] == v and not labels[t, ny, nx]:
                                labels[t, ny, nx] = n
                                stack.append((ny, nx))
                cls.append(int(v))
                area.append(a)
        offsets.append(offsets[-1] + n)
    return labels, np.asarray(offsets, np.int64), np.asarray(cls, np.int64), np.asarray(area, np.int64)


def track_align(labels, offsets, shifts):
    """-> prev_aligned, next_cropped int32 (T-1, H, W), vis_prev, vis_next int64 (N)"""
    T, H, W = labels.shape
    N = int(offsets[-1])
    prev, nxt = np.zeros((T - 1, H, W), np.int32), np.zeros((T - 1, H, W), np.int32)
    vp, vn = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for b in range(T - 1):
        sy, sx = int(shifts[b][0]), int(shifts[b][1])
        y0, y1, x0, x1 = max(0, sy), min(H, H + sy), max(0, sx), min(W, W + sx)      # q with q - s inside the frame
        if y0 < y1 and x0 < x1:
            prev[b, y0:y1, x0:x1] = labels[b, y0 - sy:y1 - sy, x0 - sx:x1 - sx]
            nxt[b, y0:y1, x0:x1] = labels[b + 1, y0:y1, x0:x1]
        for lab, cnt in zip(*np.unique(prev[b], return_counts=True)):
            if lab > 0:
                vp[offsets[b] + lab - 1] = cnt
        for lab, cnt in zip(*np.unique(nxt[b], return_counts=True)):
            if lab > 0:
                vn[offsets[b + 1] + lab - 1] = cnt
    return prev, nxt, vp, vn


def link_objects(labels, offsets, class_id, shifts, iou=0.3, scores=None, variant=None):
    """int64 (N): the batch-wide index of every object's predecessor in the frame before, or -1.  Per pair the objects of the next
    frame are visited in list order (or by descending score, ties to the smaller index); each takes the unused object of the previous
    frame of its class with the largest IoU = inter / (visible_p + visible_n - inter) on the common rectangle (ties: the smaller
    index) if that IoU is > 0 and >= iou.  variant 'whole': the areas of the whole objects in the place of the visible ones."""
    T = labels.shape[0]
    prev, nxt, vp, vn = track_align(labels, offsets, shifts)
    if variant == "whole":
        whole = np.concatenate([np.bincount(labels[t].ravel(), minlength=int(offsets[t + 1] - offsets[t]) + 1)[1:] for t in range(T)]).astype(np.int64)
        vp = vn = whole
    link = np.full(int(offsets[-1]), -1, np.int64)
    for b in range(T - 1):
        g0, p0, n_next = int(offsets[b]), int(offsets[b + 1]), int(offsets[b + 2] - offsets[b + 1])
        used = set()
        order = list(range(n_next))
        if scores is not None:
            order.sort(key=lambda i: (-float(scores[p0 + i]), i))
        both = (prev[b] > 0) & (nxt[b] > 0)
        pairs = {}
        for a, c in zip(prev[b][both].tolist(), nxt[b][both].tolist()):
            pairs[(c, a)] = pairs.get((c, a), 0) + 1
        for i in order:
            best, bj = 0.0, -1
            for (c, a), inter in sorted(pairs.items()):
                g = g0 + a - 1
                if c != i + 1 or g in used or class_id[g] != class_id[p0 + i]:
                    continue
                v = inter / (int(vn[p0 + i]) + int(vp[g]) - inter)
                if v > best:
                    best, bj = v, g
            if bj >= 0 and best >= iou:
                used.add(bj)
                link[p0 + i] = bj
    return link


def label_batch(classmap: np.ndarray, connectivity: int = 2):
    """label_frames' labels, offsets and class_id by the object tests' vectorised oracle (tests/objects_oracle.py), for maps too big or
    too full for label_frames' Python flood fill, and for 4-connected objects"""
    import objects_oracle as OO
    labels = np.stack([OO.label(m, connectivity) for m in classmap])
    offsets = np.concatenate([[0], np.cumsum([int(lab.max()) for lab in labels])]).astype(np.int64)
    cls = np.concatenate([OO.stats(lab, m)[0] for lab, m in zip(labels, classmap)]).astype(np.int64)
    return labels, offsets, cls


def track_ids(offsets, link, class_id, first_ids=None, next_id=0, capacity=None, object_capacity=None, variant=None):
    """-> (track_id int64 (N), next_id, lengths {id: frames}, classes {id: class of the first object}, status).  capacity: of the
    per-track arrays (status bit 1: an id reached it; its track is not recorded, track_id still carries it).  object_capacity: of the
    per-object arrays (status bit 2: the objects at an index past it were left out: no id, no count, no fresh id spent on them; their
    track_id stays -1).  variant 'rank256': the rank of a fresh object restarts with every 256th object of its frame."""
    T = len(offsets) - 1
    tid = np.full(int(offsets[-1]), -1, np.int64)
    lengths, classes, status = {}, {}, 0
    for t in range(T):
        end = int(offsets[t + 1])
        if object_capacity is not None and end > object_capacity:
            end, status = max(int(object_capacity), int(offsets[t])), status | 2
        frame_next = next_id
        for i in range(int(offsets[t]), end):
            fresh = False
            if variant == "rank256" and (i - int(offsets[t])) % 256 == 0:
                next_id = frame_next                                   # the fresh ids so far are handed out again
            if t == 0 and first_ids is not None:
                tid[i] = first_ids[i]
                continue
            if t > 0 and link[i] >= 0:
                tid[i] = tid[link[i]]
            else:
                tid[i], next_id, fresh = next_id, next_id + 1, True
            k = int(tid[i])
            if capacity is not None and k >= capacity:
                status |= 1
                continue
            lengths[k] = lengths.get(k, 0) + 1
            if fresh:
                classes[k] = int(class_id[i])
    return tid, next_id, lengths, classes, status
