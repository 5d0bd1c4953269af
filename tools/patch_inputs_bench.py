"""The graph branch's inputs for one training batch, one process, one GPU: B = 8 RGB images of 512 x 512, patch 16.

  fused:     mgunet.patch_node_features(images_u8, 16, images=x) (one memset + three launches) and mgunet.patch_labels(masks, 16)
             (one launch)
  composed:  what those calls replace, image by image: EdgeDetector.sobel_edges and HistogramEqualizer.equalize_histogram_rgb ->
             patch_features_u8 each, the patch pixel mean of the float image as torch ops, torch.cat; and for the labels the torch
             composition one_hot -> zero pad -> unfold sums -> argmax

HIP events around warm calls, `--rounds` interleaved rounds of `--reps` calls of each variant in ONE process; median and minimum over
the rounds' per-call times.  Prints one JSON line per measurement; the two results of each pair are compared first."""
import argparse
import functools
import statistics

import benchkit
import numpy as np
import torch
from benchkit import emit

import mgunet

per_call_ms = functools.partial(benchkit.timed, warmup=0, park=False)   # host-paced, as the composed variants are used


def composed_features(u8, x, p):
    rows = []
    edge, heq = mgunet.EdgeDetector(), mgunet.HistogramEqualizer()
    for b in range(u8.shape[0]):
        _, H, W = x[b].shape
        mean = x[b].reshape(3, H // p, p, W // p, p).mean(dim=(0, 2, 4)).reshape(-1, 1).repeat(1, 16)      # H, W multiples of p here
        sob = mgunet.patch_features_u8(edge.sobel_edges(u8[b]), p)
        eq = mgunet.patch_features_u8(heq.equalize_histogram_rgb(u8[b]), p, True)
        rows.append(torch.cat([mean, sob, eq], 1))
    return torch.cat(rows, 0)


def composed_labels(masks, p, C):
    B, H, W = masks.shape
    oh = torch.nn.functional.one_hot(masks, C).permute(0, 3, 1, 2).float()
    cnt = torch.nn.functional.avg_pool2d(oh, p, divisor_override=1)                                       # per-patch class counts
    return cnt.flatten(2).argmax(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--patch", type=int, default=16)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    B, S, p, C = args.batch, args.size, args.patch, args.classes
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    u8 = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)).to(dev)
    mean, std = torch.tensor([0.485, 0.456, 0.406], device=dev), torch.tensor([0.229, 0.224, 0.225], device=dev)
    x = ((u8.float() / 255 - mean) / std).permute(0, 3, 1, 2).contiguous()
    masks = torch.from_numpy(rng.integers(0, C, (B, S, S))).to(dev)
    pairs = {"node_features": (lambda: mgunet.patch_node_features(u8, p, images=x), lambda: composed_features(u8, x, p)),
             "labels": (lambda: mgunet.patch_labels(masks, p, C), lambda: composed_labels(masks, p, C))}
    for name, (fused, comp) in pairs.items():
        f, c = fused(), comp()
        same = torch.equal(f[:, 16:], c[:, 16:]) if name == "node_features" else torch.equal(f, c)          # the byte columns / the labels
        for fn in (fused, comp):
            per_call_ms(fn, 3)                                                                               # warm
        t = {"fused": [], "composed": []}
        for _ in range(args.rounds):
            t["fused"].append(per_call_ms(fused, args.reps))
            t["composed"].append(per_call_ms(comp, args.reps))
        emit(what="patch_inputs_" + name, B=B, H=S, W=S, patch=p, equal=bool(same),
             fused_ms_median=round(statistics.median(t["fused"]), 4), fused_ms_min=round(min(t["fused"]), 4),
             composed_ms_median=round(statistics.median(t["composed"]), 4), composed_ms_min=round(min(t["composed"]), 4))


if __name__ == "__main__":
    main()
