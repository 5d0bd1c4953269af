"""Gaussian blur at the flagship batch, one process, one GPU: B = 8 RGB images of 512 x 512, kernels 5 x 5 sigma 1 and 31 x 31 (sigma
from the size).

For each kernel, three times for the blur
  blur       GaussianSmoother.smooth on the device batch (mgu_gaussian_blur_u8, one launch)
  copy       out.copy_(img): the same bytes in and out, the floor of any kernel that reads and writes the batch once
  host       the composition the call replaces: batch to the host, a two-pass integer scipy.ndimage.correlate1d(mode='mirror') with the
             same Q8.8 weights (equal to tests/gaussian_oracle.py, checked), copy back; wall clock around a synchronise
and the same three for the fused patch column (patch 16, per channel)
  fused      patch_smooth_features_u8 (mgu_patch_smooth_mean_u8, one launch, no image written)
  composed   smooth + patch_features_u8 per image on the device
  host       the host blur above, per-patch means in numpy, copy of the rows to the device
Device times are HIP events around calls queued behind a parked stream (they time the GPU, not the host's launch rate): the median and
minimum over `--rounds` interleaved rounds.  The blur's bytes (read once + written once) over its time is printed as achieved GB/s.
The device results must equal the host's.  Prints one JSON line per measurement.  --quick: fewer rounds, one host run."""
import argparse
import functools
import statistics
import time

import benchkit
import numpy as np
import torch
from benchkit import emit
from scipy import ndimage

import mgunet

timed = functools.partial(benchkit.timed, warmup=3)


def host_blur(batch, kx, ky):
    """(B, H, W, C) uint8 numpy -> the blur in integers, two scipy passes"""
    v = ndimage.correlate1d(batch.astype(np.int32), kx.astype(np.int32), axis=2, mode="mirror")
    v = ndimage.correlate1d(v, ky.astype(np.int32), axis=1, mode="mirror")
    return ((v + 32768) >> 16).astype(np.uint8)


def host_patch_means(blurred, p):
    B, H, W, C = blurred.shape                                  # H, W multiples of p here
    s = blurred.reshape(B, H // p, p, W // p, p, C).sum((2, 4), dtype=np.int64).reshape(-1, C)
    return (s.astype(np.float64) / (float(p) * p)).astype(np.float32)


def wall(fn, runs):
    out, ts = None, []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, min(ts)


def rounds_us(fns, rounds, iters):
    """interleaved rounds of `iters` calls of every variant -> {name: (median us, min us)}"""
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(timed(fn, iters) * 1e3)
    return {k: (round(statistics.median(v), 1), round(min(v), 1)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--patch", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S, p = args.batch, args.size, args.patch
    rounds, iters, host_runs = (2, 10, 1) if args.quick else (7, 50, 3)
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, S, S, 3), dtype=np.uint8)).to(dev)
    out = torch.empty_like(img)
    nbytes = 2 * img.numel()
    for tag, ks, sigma in (("5x5_sigma1", (5, 5), 1.0), ("31x31", (31, 31), 0)):
        sm = mgunet.GaussianSmoother(ks, sigma)
        kx, ky = (np.asarray(k, np.int64) for k in sm.kernels())
        taps = sm._taps()

        def blur():
            mgunet._lib.call("mgu_gaussian_blur_u8", dev, img, B, S, S, 3, *taps, out)

        def host():
            return torch.from_numpy(host_blur(img.cpu().numpy(), kx, ky)).to(dev)

        blur()
        ref, host_s = wall(host, host_runs)
        same = bool(torch.equal(ref, out))
        us = rounds_us({"blur": blur, "copy": lambda: out.copy_(img)}, rounds, iters)
        emit(what="gaussian_blur", kernel=tag, B=B, H=S, W=S, C=3, equal_host=same, blur_us_median=us["blur"][0], blur_us_min=us["blur"][1],
             copy_us_median=us["copy"][0], copy_us_min=us["copy"][1], host_us=round(host_s * 1e6, 1),
             blur_GBps=round(nbytes / us["blur"][0] / 1e3, 1), blur_over_copy=round(us["blur"][0] / us["copy"][0], 2),
             host_over_blur=round(host_s * 1e6 / us["blur"][0], 1))
        assert same, "the device blur differs from the host composition"

        rows = torch.empty((B * (S // p) * (S // p), 3), device=dev)

        def fused():
            return mgunet.patch_smooth_features_u8(img, p, sm, True, out=rows)

        def composed():
            return torch.cat([mgunet.patch_features_u8(sm.smooth(img[b]), p, True) for b in range(B)], 0)

        def host_rows():
            return torch.from_numpy(host_patch_means(host_blur(img.cpu().numpy(), kx, ky), p)).to(dev)

        f, c = fused().clone(), composed()
        h, host_s = wall(host_rows, host_runs)
        same = bool(torch.equal(f, c) and torch.equal(f, h))
        us = rounds_us({"fused": fused, "composed": composed, "copy": lambda: out.copy_(img)}, rounds, iters)
        emit(what="patch_smooth_column", kernel=tag, B=B, H=S, W=S, patch=p, equal=same, fused_us_median=us["fused"][0],
             fused_us_min=us["fused"][1], composed_us_median=us["composed"][0], composed_us_min=us["composed"][1],
             copy_us_median=us["copy"][0], host_us=round(host_s * 1e6, 1), composed_over_fused=round(us["composed"][0] / us["fused"][0], 2),
             host_over_fused=round(host_s * 1e6 / us["fused"][0], 1))
        assert same, "the fused column differs from blur + patch means"


if __name__ == "__main__":
    main()
