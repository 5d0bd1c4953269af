"""Edge-aware refinement at the flagship batch, one process, one GPU: B = 8 images of 512 x 512 with an RGB guide, C = 2 and C = 4
classes, (radius, iterations) = (3, 1), (5, 2) and (7, 3).

  noisy      the guide is a photograph-like image: the overlapping-ellipse scene of benchkit.ellipse_scene painted with one colour per
             class (C = 4: a class per 64 x 64 cell) plus uniform noise in [-12, 12]; the probabilities are a soft version of the
             same scene moved by (2, 3) pixels, so the refinement has outlines to move
  clean      the same without the noise: inside a region every tap reads entry 0 of the range table, where under noise the 64 lanes of a
             wave read entries scattered over a few hundred -- what the LDS bank conflicts of that one lookup cost

For each: the device time of mgu_refine_probs with every output (HIP events around calls queued behind a parked stream, so they time
the GPU and not the host's launch rate) as the median of --runs timed loops of 20 calls with their spread, per call and per
iteration; as a floor, a device copy of the same bytes (the fp32 planes to the fp32 output and the guide to a buffer of its size: what
any kernel that reads the inputs once and writes the probabilities once must move); and the host composition the call replaces: the
probabilities and the guide copied to the host and the numpy oracle (tests/refine_oracle.py), labels copied back, wall clock, once;
the device outputs must equal it (run for the noisy workload).  Prints one JSON line per measurement.  --quick: fewer iterations, no
host run."""
import argparse
import time

from benchkit import ellipse_scene, emit, median_spread  # first: benchkit sets the import path
import numpy as np
import torch

import mgunet


def scene(B, H, W, C, seed, noise):
    """(probabilities float32 (B, H, W, C), guide uint8 (B, H, W, 3))"""
    rng = np.random.RandomState(seed)
    g = ellipse_scene(B, H, W, seed)
    if C > 2:
        cell = rng.randint(1, C, (B, H // 64 + 1, W // 64 + 1))
        g *= np.kron(cell, np.ones((64, 64), np.int64))[:, :H, :W]
    colours = rng.randint(30, 226, (C, 3))
    guide = np.clip(colours[g] + rng.randint(-noise, noise + 1, (B, H, W, 3)), 0, 255).astype(np.uint8)
    moved = np.zeros_like(g)
    moved[:, 2:, 3:] = g[:, :-2, :-3]
    logit = 3.0 * np.eye(C)[moved] + rng.standard_normal((B, H, W, C))
    e = np.exp(logit - logit.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32), guide


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import refine_oracle as R
    dev = torch.device("cuda:0")
    B, H, W = 8, 512, 512
    iters, runs = (3, 2) if args.quick else (20, args.runs)
    for C in (2, 4):
        for tag, noise in (("noisy", 12), ("clean", 0)):
            x, guide = scene(B, H, W, C, 1, noise)
            xt, gt = torch.from_numpy(x).to(dev).permute(0, 3, 1, 2), torch.from_numpy(guide).to(dev)
            out, gout = torch.empty((B, H, W, C), device=dev), torch.empty_like(gt)
            src = xt.permute(0, 2, 3, 1)

            def copy():
                out.copy_(src)
                gout.copy_(gt)

            cmed, clo, chi = median_spread(copy, iters, runs)
            for r, T in ((3, 1), (5, 2), (7, 3)):
                ref = mgunet.EdgeRefiner(r, 3.0, 12.0, T)
                run = lambda: ref(xt, gt, return_changed=True)  # noqa: E731
                probs, labels, conf, changed = run()
                emit(what="workload", workload=tag, C=C, B=B, H=H, W=W, G=3, radius=r, iterations=T, sigma_space=3.0, sigma_color=12.0,
                     shift=ref.tables[2], changed_pixels=int(changed.sum()))
                med, lo, hi = median_spread(run, iters, runs)
                emit(what="device", workload=tag, C=C, radius=r, iterations=T, refine_us={"median": med, "min": lo, "max": hi},
                     per_iteration_us=round(med / T, 1), copy_us={"median": cmed, "min": clo, "max": chi}, refine_over_copy=round(med / cmed, 1), loops=runs, iters=iters)
                if not args.quick and tag == "noisy":
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    want = R.refine(src.cpu().numpy(), gt.cpu().numpy(), *ref.tables, T)
                    back = torch.from_numpy(want[1]).to(dev)
                    torch.cuda.synchronize()
                    sec = time.perf_counter() - t0
                    same = (torch.equal(back, labels) and np.array_equal(probs.permute(0, 2, 3, 1).cpu().numpy(), want[0])
                            and np.array_equal(conf.cpu().numpy(), want[2]) and np.array_equal(changed.cpu().numpy(), want[3]))
                    emit(what="host_composition", workload=tag, C=C, radius=r, iterations=T, us=round(sec * 1e6, 1), same_outputs=same,
                         host_over_device=round(sec * 1e6 / med, 1))
                    assert same, "the device outputs differ from the numpy oracle"


if __name__ == "__main__":
    main()
