"""The graph cut at the two patch-graph workloads, one process, one GPU:

  headline   B = 8 graphs on a 32 x 32 grid   (the flagship batch: 8 x 512^2 at patch 16)
  c4         B = 32 graphs on a 64 x 64 grid  (32 x 1024^2 at patch 16: the largest graph one workgroup's LDS holds)

with synthetic blobby priors (a few soft discs per image), an intensity that follows them and 64 random feature columns.  For each
workload: the capacities launch, then the solve for every relabel period R x workgroup size, with the rounds each graph took.  Times
are HIP events around calls that were all queued behind a parked stream, so they time the GPU and not the host's launch rate; the
solve is one launch, so its time is the kernel's.  Prints one JSON line per measurement.  --quick: fewer iterations and settings."""
import argparse
import functools

import benchkit
import numpy as np
import torch
from benchkit import emit

import mgunet

timed = functools.partial(benchkit.timed, warmup=3)

def grid_edges(H, W):
    idx = np.arange(H * W).reshape(H, W)
    a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])]).astype(np.int64)


def blobby(B, H, W, D, seed):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    pri, inten = [], []
    for _ in range(B):
        f = -1.5 + 0.8 * rng.randn(H, W)
        for _ in range(6):
            cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.08, 0.25) * max(H, W)
            f += 4.0 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * r * r))
        p = 1.0 / (1.0 + np.exp(-f))
        pri.append(p.ravel())
        inten.append(np.clip(60 + 120 * p + 12 * rng.randn(H, W), 0, 255).ravel())
    feats = rng.randn(B * H * W, D) * (0.7 / np.sqrt(D))
    return [np.concatenate(a).astype(np.float32) for a in (pri, inten)] + [feats.astype(np.float32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--smoothness", type=float, default=2.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    iters = 5 if args.quick else 20
    periods = (8, 32) if args.quick else (2, 4, 8, 16, 32, 64, 1 << 30)
    sizes = (256, 1024) if args.quick else (128, 256, 512, 1024)
    for tag, B, H, W in (("headline", 8, 32, 32), ("c4", 32, 64, 64)):
        N, D = H * W, 64
        ei = torch.from_numpy(grid_edges(H, W)).to(dev)
        prior, inten, feats = (torch.from_numpy(a).to(dev) for a in blobby(B, H, W, D, 1))
        kw = dict(smoothness=args.smoothness, batch=B)
        caps = mgunet.cut_capacities(prior, ei, inten, feats, **kw)
        ref = mgunet.graph_cut(ei, *caps, batch=B).check()
        t_cap = timed(lambda: mgunet.cut_capacities(prior, ei, inten, feats, **kw), iters)
        emit(what="capacities", workload=tag, B=B, grid=[H, W], N=N, E=int(ei.shape[1]), D=D, us=round(t_cap * 1e3, 1),
             foreground=round(float(ref.labels.float().mean()), 3))
        for R in periods if tag == "headline" else [R for R in periods if R < 1 << 30]:   # no global relabel: thousands of rounds
            for T in sizes:
                cut = mgunet.graph_cut(ei, *caps, batch=B, relabel_period=R, threads=T)
                ok = bool(torch.equal(cut.labels, ref.labels) and torch.equal(cut.flow, ref.flow) and int(cut.converged.min()) == 1)
                ms = timed(lambda: mgunet.graph_cut(ei, *caps, batch=B, relabel_period=R, threads=T), iters)
                r = cut.rounds.cpu().numpy()
                emit(what="solve", workload=tag, R=R if R < 1 << 30 else "never", threads=T, us=round(ms * 1e3, 1),
                     rounds_min=int(r.min()), rounds_mean=round(float(r.mean()), 1), rounds_max=int(r.max()), same_cut=ok)
        d = mgunet.graph_cut(ei, *caps, batch=B)
        emit(what="solve_default", workload=tag, us=round(timed(lambda: mgunet.graph_cut(ei, *caps, batch=B), iters) * 1e3, 1),
             rounds_max=int(d.rounds.max()), capacities_plus_solve_us=round(t_cap * 1e3 + timed(lambda: mgunet.graph_cut(ei, *caps, batch=B), iters) * 1e3, 1))


if __name__ == "__main__":
    main()
