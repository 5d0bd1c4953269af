"""Boundary evaluation at the flagship batch, one process, one GPU: B = 8 images of 512 x 512, C = 2 and C = 4 classes.

  scene      the overlapping-ellipse scene of benchkit.ellipse_scene (C = 4: a class per 64 x 64 cell) as the target against a copy
             shifted by (2, 3) pixels as the prediction
  worst      the prediction is a checkerboard of 2 x 2 blocks -- every foreground pixel is a boundary pixel -- and the target one
             small object in the far corner: every query pixel walks until it has covered its distance to that corner

For each: the device time of mgu_boundary_tables on the class maps (HIP events around calls queued behind a parked stream, so they
time the GPU and not the host's launch rate), as the median of --runs timed loops with their spread, and, as a scale, of
mgunet.distance_transform of the same 2B planes.  Also the host composition the call replaces: both maps copied to the host and the
scipy oracle of the tables (tests/boundary_oracle.py), nothing copied back, wall clock, once; the device tables must equal it.  Prints
one JSON line per measurement.  --quick: fewer iterations, no host run."""
import argparse
import time

from benchkit import ellipse_scene, emit, median_spread  # first: benchkit sets the import path
import numpy as np
import torch

import mgunet
from mgunet import boundary


def shifted_scene(B, H, W, C, seed):
    """(prediction, target): the ellipse scene, a class per 64 x 64 cell for C > 2, and the same map moved by (2, 3)"""
    rng = np.random.RandomState(seed)
    g = ellipse_scene(B, H, W, seed)
    if C > 2:
        cell = rng.randint(1, C, (B, H // 64 + 1, W // 64 + 1))
        g *= np.kron(cell, np.ones((64, 64), np.int64))[:, :H, :W]
    p = np.zeros_like(g)
    p[:, 2:, 3:] = g[:, :-2, :-3]
    return p, g


def worst_scene(B, H, W, C):
    yy, xx = np.mgrid[0:H, 0:W]
    p = np.zeros((B, H, W), np.int64)
    p[:] = np.where((yy // 2 + xx // 2) % 2 == 0, 1 + (xx // 128) % (C - 1), 0)
    g = np.zeros((B, H, W), np.int64)
    for c in range(1, C):
        g[:, H - 8 * c:H - 8 * c + 6, W - 8:W - 2] = c
    return p, g


def host_tables(p_dev, g_dev, C, max_d2, band_r2):
    """The composition the device call replaces; returns (tables, seconds)."""
    import boundary_oracle as K
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = K.tables(p_dev.cpu().numpy(), g_dev.cpu().numpy(), C, max_d2, band_r2)
    return ref, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-distance", type=float, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = 8, 512, 512
    iters, runs = (3, 2) if args.quick else (20, args.runs)
    max_d2, band_r2 = boundary._max_d2(args.max_distance), boundary._band_r2(None, H, W)
    for C in (2, 4):
        for tag, (p, g) in (("scene", shifted_scene(B, H, W, C, 1)), ("worst", worst_scene(B, H, W, C))):
            p, g = torch.from_numpy(p).to(dev), torch.from_numpy(g).to(dev)
            planes = torch.cat([p, g]).to(torch.int32)
            run = lambda: boundary._tables(p, 0, g, B, H, W, 0, C, max_d2, band_r2)  # noqa: E731
            hist, stats, band = run()
            emit(what="workload", workload=tag, C=C, B=B, H=H, W=W, max_d2=max_d2, band_r2=band_r2,
                 boundary_pixels=stats[..., 0].sum((0, 1)).tolist(), unmatched=int(stats[..., 1].sum()), beyond_max_d2=int(hist[..., -1].sum()),
                 max_d2_seen=int(stats[..., 2].max()))
            med, lo, hi = median_spread(run, iters, runs)
            dmed, dlo, dhi = median_spread(lambda: mgunet.distance_transform(planes), iters, runs)
            emit(what="device", workload=tag, C=C, boundary_tables_us={"median": med, "min": lo, "max": hi},
                 distance_transform_2B_us={"median": dmed, "min": dlo, "max": dhi}, tables_over_edt=round(med / dmed, 2), loops=runs, iters=iters)
            if not args.quick:
                ref, sec = host_tables(p, g, C, max_d2, band_r2)
                same = all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((hist, stats, band), ref))
                emit(what="host_composition", workload=tag, C=C, us=round(sec * 1e6, 1), same_tables=same, host_over_device=round(sec * 1e6 / med, 1))
                assert same, "the device tables differ from the host composition"


if __name__ == "__main__":
    main()
