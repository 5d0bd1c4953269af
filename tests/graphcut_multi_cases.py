"""Inputs of the K-label graph-cut tests, shared by the CPU tier (oracle against scipy and brute force) and the GPU tier (kernel against
the oracle): numpy only.  A case is (N, coo (2, E) int64, costs (N, K) int64, cap_edge (E,) int64 symmetric, init (N,) or None)."""
import functools

import numpy as np

import graphcut_cases as GC
import graphcut_multi_oracle as GMO
import graphcut_oracle as GO

MULTI_CASES = ["n1k3", "k1", "tiepair", "zero16", "grid5x7", "grid16", "grid33x31", "grid64x32", "random200", "full64", "init16"]


def class_maps(H, W, K, seed, blobs=3):
    """K class-probability maps (softmax of noisy soft discs), (H*W, K) float32, and an intensity (0..255) that follows the classes"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    s = 0.8 * rng.randn(K, H, W)
    for k in range(K):
        for _ in range(blobs):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.1, 0.3) * max(H, W)
            s[k] += 3.0 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
    p = np.exp(s - s.max(0))
    p /= p.sum(0)
    level = (p * np.arange(K)[:, None, None]).sum(0) / max(K - 1, 1)
    inten = np.clip(40 + 170 * level + 12 * rng.randn(H, W), 0, 255)
    return p.reshape(K, -1).T.astype(np.float32).copy(), inten.ravel().astype(np.float32)


def grid_multi(H, W, K, seed, topo_seed=None, smoothness=2.0):
    coo = GC.grid_edges(H, W, topo_seed)
    p, inten = class_maps(H, W, K, seed)
    ce = GO.capacities(np.full(H * W, 0.5), coo, intensity=inten, sigma_intensity=10.0, smoothness=smoothness)[2]
    return H * W, coo, GMO.label_costs(p), ce, None


def symmetrised(coo, ce):
    """every arc gets the capacity of its pair's lower -> higher arc"""
    pos = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(*coo))}
    return np.array([ce[pos[(min(int(a), int(b)), max(int(a), int(b)))]] for a, b in zip(*coo)], np.int64)


@functools.lru_cache(maxsize=None)
def multi_case(name):
    if name == "n1k3":
        return 1, np.zeros((2, 0), np.int64), np.array([[7, 3, 5]], np.int64), np.zeros(0, np.int64), None
    if name == "k1":
        N, coo, U, ce, _ = grid_multi(5, 7, 3, 21, 4)
        return N, coo, U[:, :1].copy(), ce, None
    if name == "tiepair":   # start [0, 1] costs 4; [0, 0] and [1, 1] cost 4 as well: both moves tie, and a tie is dropped
        return 2, np.array([[0, 1], [1, 0]], np.int64), np.array([[0, 4], [4, 0]], np.int64), np.array([4, 4], np.int64), None
    if name == "zero16":    # nothing costs anything: every move proposes all-alpha at equal energy
        coo = GC.grid_edges(16, 16, 12)
        return 256, coo, np.zeros((256, 3), np.int64), np.zeros(coo.shape[1], np.int64), None
    if name == "grid5x7":
        return grid_multi(5, 7, 3, 21, 4)
    if name == "grid16":
        return grid_multi(16, 16, 4, 22, 12)
    if name == "grid16b":   # the topology of grid16 and zero16, other data
        return grid_multi(16, 16, 3, 27, 12, smoothness=1.0)
    if name == "grid33x31":
        return grid_multi(33, 31, 5, 23, 6)
    if name == "grid64x32":
        return grid_multi(64, 32, 3, 24, 7)
    if name == "random200":
        N, coo, _, _, ce = GC.solver_case("random200")
        rng = np.random.RandomState(31)
        U = rng.randint(0, 6000, (N, 6)) * (rng.rand(N, 6) < 0.7)
        return N, coo, U.astype(np.int64), symmetrised(coo, ce), None
    if name == "full64":
        return grid_multi(64, 64, 4, 25, 8)
    if name == "init16":    # a start of the caller's: stripes, with values >= K that fall back to the node's cheapest label
        N, coo, U, ce, _ = grid_multi(16, 16, 4, 22, 12)
        init = (np.arange(N) // 16 % 4).astype(np.int64)
        init[::7] = 4
        init[3::11] = 255
        return N, coo, U, ce, init
    if name == "binary16":  # the binary case "grid16" as a 2-label problem from the all-background start
        N, coo, cs, ct, ce = GC.solver_case("grid16")
        return N, coo, np.stack([cs, ct], 1).astype(np.int64), ce, np.zeros(N, np.int64)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expanded(name, max_cycles=32):
    """the oracle's result of a case with the per-move trace, computed once"""
    N, coo, U, ce, init = multi_case(name)
    trace = []
    got = GMO.expand(N, coo, U, ce, init=init, max_cycles=max_cycles, trace=trace)
    got["trace"] = trace
    return got
