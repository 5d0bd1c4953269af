"""Numpy oracle of the graph cut (csrc/graphcut.hip, mgunet/graphcut.py): the energy's capacities in float64, an exact integer max
flow by the kernel's own schedule (lock-step push-relabel with periodic global relabelling, so the round counts are comparable), the
canonical labels (foreground iff the sink is not reachable in the residual graph) and E(S) of any labelling.  No scipy, no torch."""
import math

import numpy as np

CAP_MAX = 1 << 20
INT_MAX = (1 << 31) - 1


def quant(x, unit=1024.0):
    """q(x) = min(rint(x * unit), 2^20) (round half to even, as lrintf), never negative"""
    return np.minimum(np.rint(np.maximum(np.asarray(x, np.float64) * float(unit), 0.0)), CAP_MAX).astype(np.int64)


def prior_from_counts(counts, fg):
    c = np.asarray(counts, np.int64)
    return (c[..., fg] + 1.0) / (c.sum(-1) + 2.0)


def capacities(prior, coo, intensity=None, features=None, gamma=0.5, sigma_intensity=10.0, sigma_features=1.0, smoothness=1.0, unit=1024.0):
    """One graph in float64: prior (N,) probabilities, coo (2, E), intensity (N,), features (N, D) -> cap_source, cap_sink (N,),
    cap_edge (E,) int64."""
    p = np.clip(np.asarray(prior, np.float64), 1e-6, 1.0 - 1e-6)
    cap_source, cap_sink = quant(-np.log1p(-p), unit), quant(-np.log(p), unit)
    u, v = np.asarray(coo[0]), np.asarray(coo[1])
    w = np.zeros(u.shape[0], np.float64)
    if intensity is not None:
        i = np.asarray(intensity, np.float64)
        w += np.exp(-(i[u] - i[v]) ** 2 / (2.0 * sigma_intensity ** 2))
    if features is not None:
        f = np.asarray(features, np.float64)
        w += gamma * np.exp(-((f[u] - f[v]) ** 2).sum(1) / (2.0 * sigma_features ** 2))
    return cap_source, cap_sink, quant(smoothness * w, unit)


def csr_by_source(coo, N):
    """Stable sort by source: rowptr (N+1), col, perm (CSR position -> COO index), rev (CSR position of the reverse arc).
    Raises ValueError on a self loop, a duplicate edge or a missing reverse edge."""
    u, v = np.asarray(coo[0], np.int64), np.asarray(coo[1], np.int64)
    if np.any(u == v):
        raise ValueError("self loop")
    perm = np.argsort(u, kind="stable")
    col = v[perm]
    rowptr = np.zeros(N + 1, np.int64)
    np.add.at(rowptr, u + 1, 1)
    rowptr = np.cumsum(rowptr)
    pos = {}
    for p in range(len(perm)):
        key = (int(u[perm[p]]), int(col[p]))
        if key in pos:
            raise ValueError("duplicate edge")
        pos[key] = p
    rev = np.empty(len(perm), np.int64)
    for (a, b), p in pos.items():
        if (b, a) not in pos:
            raise ValueError("missing reverse edge")
        rev[p] = pos[(b, a)]
    return rowptr, col, perm, rev


def _bfs(N, row, col, cap, sres):
    """exact residual distance to the sink, N + 1 where it cannot be reached"""
    far = N + 1
    dist = np.where(sres > 0, 1, far).astype(np.int64)
    for _ in range(N):
        live = cap > 0
        new = dist.copy()
        np.minimum.at(new, row[live], dist[col[live]] + 1)
        if np.array_equal(new, dist):
            break
        dist = new
    return dist


def default_period(N):
    """the kernel's default global-relabel period: floor(sqrt(N)) within [4, 32]"""
    return max(4, min(32, math.isqrt(N)))


def solve(N, coo, cap_source, cap_sink, cap_edge, max_rounds=None, period=None):
    """-> dict(labels uint8 (N,), flow int, rounds int, converged 0 | 1).  Capacities: integers, negative ones count as 0."""
    if period is None:
        period = default_period(N)
    rowptr, col, perm, rev = csr_by_source(coo, N)
    E = len(col)
    if max_rounds is None:
        max_rounds = 8 * N + 64
    far = N + 1
    row = np.repeat(np.arange(N), np.diff(rowptr))
    slot = np.arange(E) - rowptr[row]
    slots = [np.nonzero(slot == j)[0] for j in range(int(slot.max()) + 1 if E else 0)]
    excess = np.maximum(np.asarray(cap_source, np.int64), 0).copy()
    sres = np.maximum(np.asarray(cap_sink, np.int64), 0).copy()
    cap = np.maximum(np.asarray(cap_edge, np.int64), 0)[perm].copy() if E else np.zeros(0, np.int64)
    h = np.zeros(N, np.int64)
    flow, rounds, converged = 0, 0, 0
    r = 0
    while True:
        if r % period == 0:
            h = np.maximum(h, _bfs(N, row, col, cap, sres))
        active = (excess > 0) & (h < far)
        if not active.any():
            converged = 1
            break
        if r >= max_rounds:
            break
        rounds += 1
        snap = np.where(active, np.minimum(excess, INT_MAX), 0)
        rem = snap.copy()
        d = np.where(h == 1, np.minimum(rem, sres), 0)
        sres -= d
        rem -= d
        flow += int(d.sum())
        for P in slots:
            u, v = row[P], col[P]
            ok = (rem[u] > 0) & (h[u] == h[v] + 1) & (cap[P] > 0)
            P, u, v = P[ok], u[ok], v[ok]
            d = np.minimum(rem[u], cap[P])
            cap[P] -= d
            cap[rev[P]] += d
            np.add.at(excess, v, d)
            rem[u] -= d
        excess -= snap - rem
        hold = (excess > 0) & (h < far)
        m = np.where(sres > 0, 1, far).astype(np.int64)
        live = cap > 0
        np.minimum.at(m, row[live], h[col[live]] + 1)
        h = np.where(hold, np.maximum(h, np.minimum(m, far)), h)
        r += 1
    labels = (_bfs(N, row, col, cap, sres) >= far).astype(np.uint8)
    return {"labels": labels, "flow": int(flow), "rounds": rounds, "converged": converged}


def energy(labels, coo, cap_source, cap_sink, cap_edge):
    """E(S) in capacity units as a Python int"""
    lab = np.asarray(labels) != 0
    cs, ct, ce = (np.maximum(np.asarray(a, np.int64), 0) for a in (cap_source, cap_sink, cap_edge))
    u, v = np.asarray(coo[0]), np.asarray(coo[1])
    return int(ct[lab].sum()) + int(cs[~lab].sum()) + int(ce[lab[u] & ~lab[v]].sum())
