"""The K-label graph cut (alpha-expansion in one launch) at the two patch-graph workloads, K = 4, one process, one GPU:

  headline   B = 8 graphs on a 32 x 32 grid   (the flagship batch: 8 x 512^2 at patch 16)
  c4         B = 32 graphs on a 64 x 64 grid  (32 x 1024^2 at patch 16: the largest graph one workgroup's LDS holds)

with synthetic class-probability maps (softmax of a few soft discs per class), an intensity that follows them and 64 random feature
columns.  For each workload: label_costs, graph_cut_multi, and -- for comparison -- the composition the kernel replaces: the SAME move
sequence driven from the host, every move building cap_source / cap_sink / cap_edge with torch ops, one graph_cut, one energy and the
host read of the accept decision (the batch advances in lock step until every graph has seen K rejected moves in a row; its labels
and energies are checked to equal the kernel's).  The kernel's times are HIP events around calls queued behind a parked stream; the
composition synchronises every move, so it is timed by the wall clock around whole runs.  Prints one JSON line per measurement."""
import argparse
import functools

import benchkit
import numpy as np
import torch
from benchkit import emit, wall

import mgunet

timed = functools.partial(benchkit.timed, warmup=3)

def grid_edges(H, W):
    idx = np.arange(H * W).reshape(H, W)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])]).astype(np.int64)


def class_maps(B, H, W, K, D, seed):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    probs, inten = [], []
    for _ in range(B):
        s = 0.8 * rng.randn(K, H, W)
        for k in range(K):
            for _ in range(3):
                cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.1, 0.3) * max(H, W)
                s[k] += 3.0 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
        p = np.exp(s - s.max(0))
        p /= p.sum(0)
        probs.append(p.reshape(K, -1).T)
        level = (p * np.arange(K)[:, None, None]).sum(0) / (K - 1)
        inten.append(np.clip(40 + 170 * level + 12 * rng.randn(H, W), 0, 255).ravel())
    feats = rng.randn(B * H * W, D) * (0.7 / np.sqrt(D))
    return np.concatenate(probs).astype(np.float32), np.concatenate(inten).astype(np.float32), feats.astype(np.float32)


def composed(ei, U, ce, B, max_cycles=32):
    """alpha-expansion from the host: torch ops per move, graph_cut, two energies' worth of kernels and ONE host read per move"""
    N, K = U.shape[0] // B, U.shape[1]
    E = ei.shape[1]
    dev = U.device
    u, v = ei[0], ei[1]
    lower = u < v
    off_n = (torch.arange(B, device=dev) * N).repeat_interleave(E)
    gu, gv = u.repeat(B) + off_n, v.repeat(B) + off_n            # batched node ids per batched arc
    lo, hi = torch.minimum(gu, gv), torch.maximum(gu, gv)
    w = ce.clamp(0, 1 << 20).to(torch.int64)                     # cut_capacities writes both arcs of a pair bitwise equal
    lowb = lower.repeat(B)
    U64 = U.to(torch.int64)
    rows = torch.arange(B * N, device=dev)
    L = U64.argmin(1)

    def energy(lab):
        pairs = torch.zeros(B * N, dtype=torch.int64, device=dev).index_add_(0, lo, w * (lab[lo] != lab[hi]) * lowb)
        return (U64[rows, lab] + pairs).reshape(B, N).sum(1)

    en = energy(L)
    idle = torch.zeros(B, dtype=torch.int64, device=dev)
    moves = 0
    for move in range(max_cycles * K):
        alpha = move % K
        a, b = L[lo], L[hi]
        A, Bq, C = w * (a != b), w * (a != alpha), w * (b != alpha)
        cs, ct = U64[rows, L].clone(), U64[:, alpha].clone()
        ct.index_add_(0, lo, (C - A).clamp(min=0) * lowb)
        cs.index_add_(0, lo, (A - C).clamp(min=0) * lowb)
        cs.index_add_(0, hi, C * lowb)
        arc = ((Bq + C - A) * ~lowb).to(torch.int32)             # arc higher -> lower; lower -> higher carries nothing
        cut = mgunet.graph_cut(ei, cs.to(torch.int32), ct.to(torch.int32), arc, batch=B)
        cand = torch.where(cut.labels.reshape(-1) != 0, alpha, L)
        ec = energy(cand)
        better = ec < en
        take = better.repeat_interleave(N)
        L, en = torch.where(take, cand, L), torch.where(better, ec, en)
        idle = torch.where(better, 0, idle + 1)
        moves += 1
        if bool((idle >= K).all()):                              # the host read of every move
            break
    return L.reshape(B, N).to(torch.uint8), en, moves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--smoothness", type=float, default=2.0)
    ap.add_argument("--labels", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    iters = 5 if args.quick else 20
    K = args.labels
    for tag, B, H, W in (("headline", 8, 32, 32), ("c4", 32, 64, 64)):
        N, D = H * W, 64
        ei = torch.from_numpy(grid_edges(H, W)).to(dev)
        prob, inten, feats = (torch.from_numpy(a).to(dev) for a in class_maps(B, H, W, K, D, 1))
        ce = mgunet.cut_capacities(torch.full((B * N,), 0.5, device=dev), ei, inten, feats, smoothness=args.smoothness, batch=B)[2]
        U = mgunet.label_costs(prob, batch=B)
        ref = mgunet.graph_cut_multi(ei, U, ce, batch=B).check()
        start = mgunet.cut_energy_multi(U.argmin(1), ei, U, ce, batch=B)
        t_costs = timed(lambda: mgunet.label_costs(prob, batch=B), iters)
        t_cut = timed(lambda: mgunet.graph_cut_multi(ei, U, ce, batch=B), iters)
        t_both = timed(lambda: mgunet.graph_cut_multi(ei, mgunet.label_costs(prob, batch=B), ce, batch=B), iters)
        m, r = ref.moves.cpu().numpy(), ref.rounds.cpu().numpy()
        emit(what="expansion", workload=tag, B=B, grid=[H, W], N=N, E=int(ei.shape[1]), K=K, label_costs_us=round(t_costs * 1e3, 1),
             graph_cut_multi_us=round(t_cut * 1e3, 1), label_costs_plus_graph_cut_multi_us=round(t_both * 1e3, 1), moves_min=int(m.min()),
             moves_max=int(m.max()), accepted_mean=round(float(ref.accepted.float().mean()), 1), rounds_mean=round(float(r.mean()), 1),
             rounds_max=int(r.max()), energy_start_over_end=round(float(start.sum()) / max(float(ref.energy.sum()), 1.0), 3))
        L, en, moves = composed(ei, U, ce, B)
        same = bool(torch.equal(L, ref.labels) and torch.equal(en, ref.energy))
        t_comp = wall(lambda: composed(ei, U, ce, B), 2 if args.quick else 5, 1)
        emit(what="composed", workload=tag, moves=moves, us=round(t_comp * 1e3, 1), same_labels_and_energy=same,
             over_kernel=round(t_comp / t_cut, 1))


if __name__ == "__main__":
    main()
