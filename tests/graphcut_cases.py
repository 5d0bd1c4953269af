"""Inputs of the graph-cut tests, shared by the CPU tier (oracle against scipy) and the GPU tier (kernel against the oracle): numpy
only.  A solver case is (N, coo (2, E) int64, cap_source, cap_sink, cap_edge) with int64 capacity arrays in int32 range."""
import functools

import numpy as np

import graphcut_oracle as GO

SOLVER_CASES = ["n1", "n2", "isolated", "tie", "grid5x7", "grid16", "grid33x31", "random200", "zero16", "allbg16", "wide32", "wide64x32", "full64"]


def grid_edges(H, W, seed=None):
    """4-connected H x W grid, both directions of every edge; seed: the COO order shuffled (CSR rows then come out unsorted)"""
    idx = np.arange(H * W).reshape(H, W)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    coo = np.stack([np.concatenate([a, b]), np.concatenate([b, a])]).astype(np.int64)
    if seed is not None:
        coo = coo[:, np.random.RandomState(seed).permutation(coo.shape[1])]
    return coo


def blobby(H, W, seed, blobs=6):
    """a foreground probability map of a few soft discs on a noisy background, and an intensity map (0..255) that follows it"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = -1.5 + 0.8 * rng.randn(H, W)
    for _ in range(blobs):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.08, 0.25) * max(H, W)
        f += 4.0 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    p = 1.0 / (1.0 + np.exp(-f))
    inten = np.clip(60 + 120 * p + 12 * rng.randn(H, W), 0, 255)
    return p.ravel().astype(np.float32), inten.ravel().astype(np.float32)


def grid_case(H, W, seed):
    coo = grid_edges(H, W, seed)
    p, inten = blobby(H, W, seed)
    return (H * W, coo) + GO.capacities(p, coo, intensity=inten, sigma_intensity=10.0)


def wide_case(H, W):
    """every source arc 2^20 and arcs wide enough to carry all of it to two sink nodes: the excess of a node and the flow leave 32 bits"""
    N = H * W
    coo = grid_edges(H, W, 3)
    ct = np.zeros(N, np.int64)
    ct[[N // 2 + W // 2, N - 1]] = (1 << 31) - 1
    return N, coo, np.full(N, 1 << 20, np.int64), ct, np.full(coo.shape[1], 1 << 30, np.int64)


def random_case(N=200, seed=7):
    """random symmetric topology of degree <= 9 with ASYMMETRIC capacities (cap[k] != cap[rev[k]]), many of them 0"""
    rng = np.random.RandomState(seed)
    deg, pairs = np.zeros(N, int), set()
    for _ in range(4 * N):
        a, b = rng.randint(0, N, 2)
        if a != b and deg[a] < 9 and deg[b] < 9 and (min(a, b), max(a, b)) not in pairs:
            pairs.add((min(a, b), max(a, b)))
            deg[a] += 1
            deg[b] += 1
    pr = np.array(sorted(pairs)).T
    coo = np.concatenate([pr, pr[::-1]], 1).astype(np.int64)
    coo = coo[:, rng.permutation(coo.shape[1])]
    ce = rng.randint(0, 2000, coo.shape[1]) * (rng.rand(coo.shape[1]) < 0.8)
    cs = rng.randint(0, 6000, N) * (rng.rand(N) < 0.4)
    ct = rng.randint(0, 6000, N) * (rng.rand(N) < 0.4)
    return N, coo, cs.astype(np.int64), ct.astype(np.int64), ce.astype(np.int64)


@functools.lru_cache(maxsize=None)
def solver_case(name):
    if name == "n1":
        return 1, np.zeros((2, 0), np.int64), np.array([7]), np.array([3]), np.zeros(0, np.int64)
    if name == "n2":
        return 2, np.array([[0, 1], [1, 0]]), np.array([10, 0]), np.array([0, 6]), np.array([4, 4])
    if name == "isolated":
        return 4, np.array([[0, 1, 1, 2], [1, 0, 2, 1]]), np.array([9, 0, 2, 5]), np.array([0, 3, 8, 9]), np.array([6, 6, 2, 2])
    if name == "tie":   # s - a - b - t, every capacity 5: three cuts of cost 5, the canonical one keeps both nodes in the foreground
        return 2, np.array([[0, 1], [1, 0]]), np.array([5, 0]), np.array([0, 5]), np.array([5, 5])
    if name == "grid5x7":
        return grid_case(5, 7, 11)
    if name == "grid16":
        return grid_case(16, 16, 12)
    if name == "grid33x31":
        return grid_case(33, 31, 13)
    if name == "random200":
        return random_case()
    if name in ("zero16", "allbg16"):
        N, coo, cs, ct, ce = grid_case(16, 16, 12)
        if name == "zero16":    # flow 0, every node foreground by the tie rule
            return N, coo, cs * 0, ct * 0, ce * 0
        return N, coo, cs, np.full(N, 1 << 30, np.int64), ce     # every node background
    if name == "wide32":
        return wide_case(32, 32)
    if name == "wide64x32":
        return wide_case(64, 32)
    if name == "full64":
        return grid_case(64, 64, 14)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def solved(name):
    """the oracle's result of a case, computed once"""
    N, coo, cs, ct, ce = solver_case(name)
    return GO.solve(N, coo, cs, ct, ce)
