"""CLAHE at the flagship batch, one process, one GPU: B = 8 images of 512 x 512 with 3 channels and with 1, grid 8 x 8, clip limit 2.0,
on a scene (a bright graded sky over a dark noisy canopy) and on a uniform image (every count of a tile on one bin: the worst case of
the histogram's atomics and the largest clip).

  both       mgu_clahe_u8 (two launches), HIP events around calls queued behind a parked stream
  lut, apply each launch between its own event pair (mgu_profile_enable: the records csrc/clahe.hip makes around its launches); an
             event pair around one short launch also holds the gap to its neighbours, so the two add up to more than `both`
  copy       out.copy_(img): the same bytes in and out, the floor of any kernel that reads and writes the batch once
  global     mgu_equalize_hist_rgb_u8 once per image: the one-table equalisation a user composes today (3 channels)
  host       tests/clahe_oracle.py in numpy on the host batch (its result must equal the device's), wall clock, once
and for the fused patch column (patch 16, per channel, 3 channels)
  fused      patch_clahe_features_u8 (mgu_patch_clahe_mean_u8, two launches, no image written)
  composed   CLAHE.apply + patch_features_u8 per image on the device
Device times are the median, minimum and maximum of `--runs` loops of `--iters` calls.  Prints one JSON line per measurement and, with
--out, writes the same lines to that file."""
import argparse
import json
import statistics
import time

import benchkit
import numpy as np
import torch
from benchkit import median_spread

import clahe_oracle as O
import mgunet
from mgunet import _lib

LINES = []


def line(**kw):
    benchkit.emit(**kw)
    LINES.append(json.dumps(kw))


def scene(B, S, ch, seed):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64) / S
    out = np.zeros((B, S, S, ch), np.uint8)
    for b in range(B):
        horizon = 0.35 + 0.1 * np.sin(2 * np.pi * (xx * (1 + b % 3) + 0.1 * b))
        sky = 235 - 60 * yy
        canopy = 45 + 25 * np.sin(9 * xx + b) * np.cos(7 * yy) + rng.normal(0, 12, (S, S))
        grey = np.where(yy < horizon, sky + rng.normal(0, 2, (S, S)), canopy)
        for c in range(ch):
            out[b, :, :, c] = np.clip(grey * (1.0 - 0.08 * c) + 6 * c, 0, 255).astype(np.uint8)
    return out


def per_launch_us(ctx, fn, iters, runs):
    """{kernel name: median us per launch} from the context's event records"""
    per = {}
    for _ in range(runs):
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
        for _ in range(iters):
            fn()
        for k in _lib.read_kernel_stats(ctx):
            per.setdefault(k["name"], []).append(k["ms"] * 1e3 / k["launches"])
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return {k: round(statistics.median(v), 1) for k, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--clip", type=float, default=2.0)
    ap.add_argument("--patch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S, G, clip, p = args.batch, args.size, args.grid, args.clip, args.patch
    ctx = _lib.context(dev)
    clahe = mgunet.CLAHE(clip, (G, G))
    for ch in (3, 1):
        for content in ("scene", "uniform"):
            host_img = scene(B, S, ch, 7) if content == "scene" else np.full((B, S, S, ch), 77, np.uint8)
            img = torch.from_numpy(host_img).to(dev)
            out = torch.empty_like(img)

            def both():
                _lib.call("mgu_clahe_u8", dev, img, B, S, S, ch, G, G, clip, out, None)

            both()
            t0 = time.perf_counter()
            want, _luts = O.clahe(host_img, G, G, clip)
            host_s = time.perf_counter() - t0
            same = bool(np.array_equal(out.cpu().numpy(), want))
            us_both, us_copy = median_spread(both, args.iters, args.runs), median_spread(lambda: out.copy_(img), args.iters, args.runs)
            each = per_launch_us(ctx, both, args.iters, args.runs)
            rec = dict(what="clahe", content=content, B=B, H=S, W=S, C=ch, grid=G, clip=clip, equal_oracle=same, both_us_median=us_both[0],
                       both_us_min=us_both[1], both_us_max=us_both[2], lut_us=each.get("clahe_lut_kernel"), apply_us=each.get("clahe_apply_kernel"),
                       copy_us_median=us_copy[0], copy_us_min=us_copy[1], both_over_copy=round(us_both[0] / us_copy[0], 2),
                       both_GBps=round(2 * img.numel() / us_both[0] / 1e3, 1), host_oracle_us=round(host_s * 1e6, 1))
            if ch == 3:
                def global_eq():
                    for b in range(B):
                        _lib.call("mgu_equalize_hist_rgb_u8", dev, img[b], S, S, out[b])

                us_g = median_spread(global_eq, args.iters, args.runs)
                rec.update(global_per_image_us_median=us_g[0], global_per_image_us_min=us_g[1], global_over_both=round(us_g[0] / us_both[0], 2))
            line(**rec)
            assert same, "the device result differs from the oracle"
            if ch == 3:
                rows = torch.empty((B * (-(-S // p)) ** 2, 3), device=dev)

                def fused():
                    return mgunet.patch_clahe_features_u8(img, p, clahe, True, out=rows)

                def composed():
                    return torch.cat([mgunet.patch_features_u8(clahe.apply(img[b]), p, True) for b in range(B)], 0)

                f, c = fused().clone(), composed()
                same = bool(torch.equal(f, c))
                us_f, us_c = median_spread(fused, args.iters, args.runs), median_spread(composed, args.iters, args.runs)
                each = per_launch_us(ctx, fused, args.iters, args.runs)
                line(what="patch_clahe_column", content=content, B=B, H=S, W=S, patch=p, equal=same, fused_us_median=us_f[0], fused_us_min=us_f[1],
                     mean_kernel_us=each.get("patch_clahe_mean_kernel"), composed_us_median=us_c[0], composed_us_min=us_c[1],
                     composed_over_fused=round(us_c[0] / us_f[0], 2))
                assert same, "the fused column differs from CLAHE + patch means"
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
