"""Mask cleanup at the flagship batch, one process, one GPU: B = 8 images of 512 x 512, logits of C = 2 and C = 4 classes.

  scene      the overlapping-ellipse scene of benchkit.ellipse_scene (C = 4: a class per cluster) with pin holes inside the fruits and
             one-pixel spurs sticking out of them
  worst      a checkerboard of single-pixel holes: every other pixel is a background component of its own (H*W/2 roots for the fill),
             and every plane word is half set

For each: the device time of mgu_clean_masks with close r = 2 + fill + open r = 2 on the logits (argmax fused), of each stage alone,
and of mgu_connected_components on the same batch (HIP events around calls queued behind a parked stream, so they time the GPU and
not the host's launch rate), with the pixels each stage changed and the whole call's cost as a multiple of the labelling.  Also the
host composition the call replaces: the argmax map copied to the host, scipy's binary dilation / erosion per class, the background
labelled by scipy for the holes (tests/clean_oracle.py) and the copy back, wall clock, once; the device result must equal it.
Prints one JSON line per measurement.  --quick: fewer iterations, no host run."""
import argparse
import functools
import time

import benchkit
import numpy as np
import torch
from benchkit import ellipse_scene, emit, logits_of

from mgunet import objects

timed = functools.partial(benchkit.timed, warmup=3)


def defect_scene(B, H, W, C, seed):
    """the ellipse scene with a class per 64 x 64 cell (C > 2), 200 pin holes and 60 spurs of 1 x 12 pixels per image"""
    rng = np.random.RandomState(seed)
    m = ellipse_scene(B, H, W, seed)
    if C > 2:
        cell = rng.randint(1, C, (B, H // 64 + 1, W // 64 + 1))
        m *= np.kron(cell, np.ones((64, 64), np.int64))[:, :H, :W]
    for b in range(B):
        ys, xs = np.nonzero(m[b])
        pick = rng.choice(ys.size, 260, replace=False)
        for k in pick[200:]:
            x1 = min(W, xs[k] + 12)
            m[b, ys[k], xs[k]:x1] = m[b, ys[k], xs[k]]
        m[b, ys[pick[:200]], xs[pick[:200]]] = 0
    return m


def checker_scene(B, H, W, C):
    m = np.zeros((B, H, W), np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    m[:] = np.where((yy + xx) % 2 == 0, 1 + (xx // 128) % (C - 1), 0)
    return m


def host_clean(logits, C, params):
    """The composition the device call replaces; returns (int64 map on the device, seconds)."""
    import clean_oracle as K
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cmap = torch.argmax(logits, 1).cpu().numpy()
    out = torch.from_numpy(K.clean(cmap, C, *params)[0]).to(logits.device)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--radius", type=float, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = 8, 512, 512
    iters = 3 if args.quick else 30
    full = objects._clean_params(args.radius, True, 0, args.radius)
    stages = {"close": (full[0], 0, 0, 0), "fill": (0, 1, 0, 0), "open": (0, 0, 0, full[3])}
    for C in (2, 4):
        for tag, cmap in (("scene", defect_scene(B, H, W, C, 1)), ("worst", checker_scene(B, H, W, C))):
            logits = logits_of(cmap, C, dev)
            src = logits.permute(0, 2, 3, 1)
            out = torch.empty((B, H, W), device=dev, dtype=torch.int64)
            counts = torch.empty((B, 3), device=dev, dtype=torch.int64)
            labels = torch.empty((B, H, W), device=dev, dtype=torch.int32)
            n, off = torch.empty(B, device=dev, dtype=torch.int64), torch.empty(B + 1, device=dev, dtype=torch.int64)
            run = lambda p=full: objects._clean(src, 1, B, H, W, C, C, p, out, counts)  # noqa: E731
            run()
            emit(what="workload", workload=tag, C=C, B=B, H=H, W=W, close_radius_sq=full[0], open_radius_sq=full[3],
                 foreground=round(float((torch.argmax(logits, 1) > 0).float().mean()), 3), changed=counts.sum(0).tolist())
            us = {k: round(timed(lambda p=p: run(p), iters) * 1e3, 1) for k, p in stages.items()}
            us["clean_masks"] = round(timed(run, iters) * 1e3, 1)
            us["connected_components"] = round(timed(lambda: objects._label(src, 1, B, H, W, C, 2, 0, 0, 0, labels, n, off), iters) * 1e3, 1)
            emit(what="device", workload=tag, C=C, us=us, clean_over_label=round(us["clean_masks"] / us["connected_components"], 2))
            if not args.quick:
                run()
                ref, sec = host_clean(logits, C, full)
                emit(what="host_composition", workload=tag, C=C, us=round(sec * 1e6, 1), same_map=bool(torch.equal(ref, out)),
                     host_over_device=round(sec * 1e6 / us["clean_masks"], 1))
                assert torch.equal(ref, out), "the device result differs from the host composition"


if __name__ == "__main__":
    main()
