"""Numpy oracle of the K-label graph cut (csrc/graphcut.hip: mgu_graphcut_label_costs / _expand / _energy_multi): the label costs in
float64, alpha-expansion with the kernel's own move construction, move order, accept rule and -- through graphcut_oracle.solve -- round
schedule, so labels, energy, moves, accepted and rounds are all comparable bit for bit, and E(L) of any labelling.  No scipy, no torch.

    E(L) = sum_i U_i(L_i) + sum over pairs {i,j} of w_ij [L_i != L_j],   w_ij = cap_edge of the arc from the lower to the higher node id
"""
import numpy as np

import graphcut_oracle as GO

CAP_MAX = GO.CAP_MAX


def label_costs(prior, unit=1024.0):
    """(rows, K) float probabilities, or integer class counts with p = (n_k + 1) / (n_all + K) -> U (rows, K) int64"""
    a = np.asarray(prior)
    if a.dtype.kind in "iu":
        c = np.maximum(a.astype(np.int64), 0)
        p = (c + 1.0) / (c.sum(-1, keepdims=True) + float(a.shape[-1]))
    else:
        p = a.astype(np.float64)
    return GO.quant(-np.log(np.clip(p, 1e-6, 1.0)), unit)


def _clamp(a):
    return np.clip(np.asarray(a, np.int64), 0, CAP_MAX)


def pairs(coo, cap_edge):
    """(lo, hi, w, k_lo_hi, k_hi_lo): every pair once, with the COO positions of its two arcs"""
    u, v = np.asarray(coo[0], np.int64), np.asarray(coo[1], np.int64)
    k = np.nonzero(u < v)[0]
    pos = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(u, v))}
    back = np.array([pos[(int(v[i]), int(u[i]))] for i in k], np.int64) if len(k) else np.zeros(0, np.int64)
    return u[k], v[k], _clamp(cap_edge)[k] if len(k) else np.zeros(0, np.int64), k, back


def energy_multi(labels, coo, costs, cap_edge):
    """E(L) as a Python int"""
    L = np.asarray(labels, np.int64)
    U = _clamp(costs)
    u, v = np.asarray(coo[0], np.int64), np.asarray(coo[1], np.int64)
    w = _clamp(cap_edge) if len(u) else np.zeros(0, np.int64)
    cut = (u < v) & (L[u] != L[v])
    return int(U[np.arange(len(L)), L].sum()) + int(w[cut].sum())


def start_labels(costs, init=None):
    U = _clamp(costs)
    first = np.argmin(U, 1)                                # the lowest label on ties
    if init is None:
        return first.astype(np.int64)
    init = np.asarray(init, np.int64)
    return np.where(init >= U.shape[1], first, init)


def move_capacities(L, alpha, coo, costs, cap_edge, pr=None):
    """The kernel's construction of the move "x_i = 1: node i takes alpha" -> (cap_source, cap_sink, cap_edge per COO arc)"""
    U = _clamp(costs)
    N = len(L)
    lo, hi, w, k_fwd, k_back = pr if pr is not None else pairs(coo, cap_edge)
    cs, ct = U[np.arange(N), L].copy(), U[:, alpha].copy()
    a, b = L[lo], L[hi]
    A, B, C = w * (a != b), w * (a != alpha), w * (alpha != b)
    np.add.at(ct, lo, np.maximum(C - A, 0))
    np.add.at(cs, lo, np.maximum(A - C, 0))
    np.add.at(cs, hi, C)
    ce = np.zeros(np.asarray(coo).shape[1], np.int64)
    ce[k_back] = B + C - A                                 # arc hi -> lo; lo -> hi carries nothing
    return cs, ct, ce


def expand(N, coo, costs, cap_edge, init=None, max_cycles=32, max_rounds=None, period=None, trace=None):
    """-> dict(labels uint8 (N,), energy, moves, accepted, rounds, converged).  trace: a list that receives, per move,
    (labels before, alpha, labels the move proposes, accepted)."""
    U = _clamp(costs)
    K = U.shape[1]
    L = start_labels(U, init)
    pr = pairs(coo, cap_edge)
    E = energy_multi(L, coo, U, cap_edge)
    moves = accepted = rounds = idle = converged = 0
    for move in range(max_cycles * K):
        alpha = move % K
        cs, ct, ce = move_capacities(L, alpha, coo, U, cap_edge, pr)
        moves += 1
        got = GO.solve(N, coo, cs, ct, ce, max_rounds=max_rounds, period=period)
        rounds += got["rounds"]
        if not got["converged"]:
            break
        cand = np.where(got["labels"] != 0, alpha, L)
        Ec = energy_multi(cand, coo, U, cap_edge)
        ok = Ec < E
        if trace is not None:
            trace.append((L.copy(), alpha, cand.copy(), ok))
        if ok:
            L, E, idle = cand, Ec, 0
            accepted += 1
        else:
            idle += 1
            if idle >= K:
                converged = 1
                break
    return {"labels": L.astype(np.uint8), "energy": int(E), "moves": moves, "accepted": accepted, "rounds": rounds, "converged": converged}
