"""numpy / float64 restatement of tiled inference, written from its definitions and from none of mgunet.tiled's code: the per-axis
grid, the window and its normalisation, the reflect-padded gather and the weighted merge of the tiles' softmaxes."""
import math

import numpy as np


def axis_origins(L, T, o):
    """Brute force: walk the stride until a tile reaches the end, then pull the last one back so that it ends at L."""
    if L <= T:
        return [0]
    out, k = [], 0
    while k + T < L:
        out.append(k)
        k += T - o
    out.append(L - T)
    assert len(out) == math.ceil((L - T) / (T - o)) + 1
    return out


def window(T, o, name):
    i = np.arange(T, dtype=np.float64)
    if name == "flat":
        return np.ones(T)
    assert name == "ramp"
    return np.minimum(1.0, np.minimum((i + 1) / (o + 1), (T - i) / (o + 1)))


def axis_weights(L, T, o, origins, name):
    """float32 (n, T): w(i) over the sum of w(p - origin) of the tiles covering p = origin_k + i, in float64, rounded once"""
    w = window(T, o, name)
    total = np.zeros(max(L, T))
    for org in origins:
        total[org:org + T] += w
    return np.stack([w / total[org:org + T] for org in origins]).astype(np.float32)


def coverage(L, T, origins):
    """how many tiles cover each of the L image coordinates"""
    n = np.zeros(L, np.int64)
    for org in origins:
        n[org:min(org + T, L)] += 1
    return n


def gather(img, Th, Tw, oy, ox):
    """img (B, C, H, W) -> (B * len(oy) * len(ox), C, Th, Tw), image-major then row-major, through numpy's reflect padding"""
    B, C, H, W = img.shape
    pad = np.pad(img, ((0, 0), (0, 0), (0, max(0, Th - H)), (0, max(0, Tw - W))), mode="reflect")
    return np.stack([pad[b, :, y:y + Th, x:x + Tw] for b in range(B) for y in oy for x in ox])


def softmax64(logits, axis=-1):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def merge(tile_probs, B, H, W, Th, Tw, o, name):
    """tile_probs float64 (ntiles, Th, Tw, C) -> float64 (B, H, W, C): sum over the covering tiles of wn_y * wn_x * p, the weights
    being the float32 tables and their float32 product, as the contract defines them"""
    oy, ox = axis_origins(H, Th, o), axis_origins(W, Tw, o)
    wy, wx = axis_weights(H, Th, o, oy, name), axis_weights(W, Tw, o, ox, name)
    out = np.zeros((B, H, W, tile_probs.shape[-1]))
    t = 0
    for b in range(B):
        for r, y in enumerate(oy):
            for c, x in enumerate(ox):
                h, w = min(Th, H - y), min(Tw, W - x)
                wgt = (wy[r][:h, None] * wx[c][None, :w]).astype(np.float32).astype(np.float64)
                out[b, y:y + h, x:x + w] += wgt[..., None] * tile_probs[t, :h, :w]
                t += 1
    return out
