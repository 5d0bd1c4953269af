"""Tiled inference on one large photograph, one process, one GPU: a 3000 x 4000 uint8 image through the headline UNet (3 -> 2 classes,
32 features, depth 4) with tile 512, overlap 64, 8 tiles per forward.

  per chunk (HIP events, median over `reps` passes of every full chunk): gather_ms (mgu_tile_gather_u8), forward_ms (the model on the
  8 x 512^2 batch), accumulate_ms (mgu_tile_accumulate), and overhead = (gather + accumulate) / forward: what tiling adds to the
  forward it cannot avoid.
  end to end: median of a warm mgunet.predict_tiled call, and of the torch composition a user would otherwise write (normalise the
  image, then per chunk: crop, model, softmax, weighted += on a canvas and on a weight canvas; divide, argmax, amax at the end).

Prints one JSON line per measurement.  `--trace DIR` reads the kernel trace a run under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/tiled_bench.py --reps 3 --no-torch` left there and prints
the two kernels' median times with the bytes they must move (`--bytes` prints those alone; neither needs a GPU)."""
import argparse
import csv
import glob
import json
import os
import functools
import statistics

import benchkit
import numpy as np
import torch

import mgunet
from mgunet import tiled

median_ms = functools.partial(benchkit.timed_each, warmup=2)

CFG = (3, 2, 32, 4)
MEAN, STD = tiled.DEFAULT_MEAN, tiled.DEFAULT_STD


def chunk_bytes(H, W, T, o, per, C=CFG[1]):
    """Compulsory bytes per chunk of one image.  gather_u8: the tiles' bytes read once, their floats written.  accumulate: the
    in-image logits read, the canvas read where an earlier chunk already added, written where the chunk adds, labels (8) and
    confidence (4) written where the chunk holds the pixel's last tile."""
    oy, ox = tiled.tile_grid(H, W, T, o)
    first = np.full((H, W), -1, np.int64)
    last = np.full((H, W), -1, np.int64)
    t = 0
    for y in oy:
        for x in ox:
            sl = (slice(y, min(y + T, H)), slice(x, min(x + T, W)))
            first[sl] = np.where(first[sl] < 0, t, first[sl])
            last[sl] = t
            t += 1
    out = []
    for t0 in range(0, t, per):
        n = min(per, t - t0)
        touched = np.zeros((H, W), bool)
        logits = 0
        for k in range(t0, t0 + n):
            y, x = oy[k // len(ox)], ox[k % len(ox)]
            sl = (slice(y, min(y + T, H)), slice(x, min(x + T, W)))
            touched[sl] = True
            logits += (sl[0].stop - y) * (sl[1].stop - x)
        load = int((touched & (first < t0)).sum())
        done = int((touched & (last < t0 + n)).sum())
        out.append({"t0": t0, "n": n, "gather_bytes": n * T * T * 3 * (1 + 4),
                    "accumulate_bytes": logits * C * 4 + (load + int(touched.sum())) * C * 4 + done * 12})
    return out


def torch_composition(model, img_u8, T, o, per):
    """what a user writes without predict_tiled: every step a torch op on the device"""
    H, W, _ = img_u8.shape
    dev = img_u8.device
    x = ((img_u8.flip(-1).permute(2, 0, 1).float() / 255.0 - torch.tensor(MEAN, device=dev).view(3, 1, 1)) / torch.tensor(STD, device=dev).view(3, 1, 1))
    oy, ox = tiled.tile_grid(H, W, T, o)
    i = torch.arange(T, device=dev, dtype=torch.float32)
    w1 = torch.minimum(torch.ones_like(i), torch.minimum((i + 1) / (o + 1), (T - i) / (o + 1)))
    w2 = (w1[:, None] * w1[None, :])[None]
    canvas = torch.zeros((CFG[1], H, W), device=dev)
    norm = torch.zeros((1, H, W), device=dev)
    org = [(y, x0) for y in oy for x0 in ox]
    with torch.no_grad():
        for t0 in range(0, len(org), per):
            part = org[t0:t0 + per]
            batch = torch.stack([x[:, y:y + T, x0:x0 + T] for y, x0 in part])
            p = torch.softmax(model(batch)[0], 1)
            for k, (y, x0) in enumerate(part):
                canvas[:, y:y + T, x0:x0 + T] += w2 * p[k]
                norm[:, y:y + T, x0:x0 + T] += w2
        probs = canvas / norm
        return probs, probs.argmax(0), probs.amax(0)


def trace_report(root, H, W, T, o, per):
    f = max(glob.glob(f"{root}/**/*kernel_trace.csv", recursive=True), key=os.path.getmtime)
    per_kernel = {}
    for r in csv.DictReader(open(f)):
        for key in ("tile_gather_kernel", "tile_accumulate_kernel"):
            if key in r["Kernel_Name"]:
                per_kernel.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    full = [c for c in chunk_bytes(H, W, T, o, per) if c["n"] == per]
    for key, field in (("tile_gather_kernel", "gather_bytes"), ("tile_accumulate_kernel", "accumulate_bytes")):
        d = [ns for _, ns in sorted(per_kernel.get(key, []))]                  # every launch; nearly all are full chunks
        mb = statistics.mean(c[field] for c in full) / 1e6
        med = statistics.median(d) / 1e3
        print(json.dumps({"what": "tiled_kernel", "kernel": key, "calls": len(d), "median_us": round(med, 1), "min_us": round(min(d) / 1e3, 1),
                          "MB_per_full_chunk": round(mb, 1), "TB_per_s": round(mb / med, 2), "share_of_6.3_TB_per_s_copy": round(mb / med / 6.3, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=64)
    ap.add_argument("--tiles-per-batch", type=int, default=8)
    ap.add_argument("--dtype", default="float32", choices=["float32", "bfloat16"])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition")
    ap.add_argument("--bytes", action="store_true", help="print the kernels' compulsory bytes per chunk and exit (no GPU)")
    ap.add_argument("--trace", help="directory of a rocprofv3 kernel trace of this script: print the kernels' times and rates (no GPU)")
    args = ap.parse_args()
    H, W, T, o, per = args.height, args.width, args.tile, args.overlap, args.tiles_per_batch
    if args.bytes:
        for c in chunk_bytes(H, W, T, o, per):
            print(json.dumps({"what": "tiled_bytes", **c}))
        return
    if args.trace:
        trace_report(args.trace, H, W, T, o, per)
        return
    dev = torch.device("cuda:0")
    model = mgunet.UNet(*CFG, compute_dtype=getattr(torch, args.dtype)).to(dev).eval()
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    plan = tiled.TilePlan(1, H, W, T, o, "ramp", dev)
    probs = torch.empty((1, H, W, CFG[1]), device=dev)
    labels = torch.empty((1, H, W), device=dev, dtype=torch.int64)
    conf = torch.empty((1, H, W), device=dev)
    buf = torch.empty((per, 3, T, T), device=dev)
    starts = [t0 for t0 in range(0, plan.ntiles, per) if t0 + per <= plan.ntiles]
    with torch.no_grad():
        lg = model(plan.gather_u8(img[None], True, MEAN, STD, 0, per, out=buf))[0].permute(0, 2, 3, 1)
        mgunet.predict_tiled(model, img, tile=T, overlap=o, tiles_per_batch=per, bgr=True)        # every chunk's canvas state is real
        g = median_ms(lambda: [plan.gather_u8(img[None], True, MEAN, STD, t0, per, out=buf) for t0 in starts], args.reps) / len(starts)
        f = median_ms(lambda: model(buf), args.reps * 2)
        a = median_ms(lambda: [plan.accumulate(lg, t0, probs, labels, conf) for t0 in starts], args.reps) / len(starts)
        print(json.dumps({"what": "tiled_chunk", "dtype": args.dtype, "H": H, "W": W, "tile": T, "overlap": o, "tiles_per_batch": per,
                          "tiles": plan.ntiles, "full_chunks": len(starts), "gather_ms": round(g, 4), "forward_ms": round(f, 3),
                          "accumulate_ms": round(a, 4), "overhead_over_forward": round((g + a) / f, 4)}), flush=True)
        e2e = median_ms(lambda: mgunet.predict_tiled(model, img, tile=T, overlap=o, tiles_per_batch=per, bgr=True), args.reps)
        row = {"what": "tiled_e2e", "dtype": args.dtype, "predict_tiled_ms": round(e2e, 2)}
        if not args.no_torch:
            ref = torch_composition(model, img, T, o, per)
            got = mgunet.predict_tiled(model, img, tile=T, overlap=o, tiles_per_batch=per, bgr=True)
            row["max_abs_diff_vs_torch"] = float((got[0][0] - ref[0]).abs().max())
            row["torch_composition_ms"] = round(median_ms(lambda: torch_composition(model, img, T, o, per), args.reps), 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
