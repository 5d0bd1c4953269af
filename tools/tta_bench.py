"""Test-time augmentation against the plain forward, one process, one GPU: the headline UNet (3 -> 2 classes, 32 features, depth 4)
at 512^2, B = 1 and 8, fp32 and bf16 storage, transforms none / hflip / d4.

  tta_ms: median of a warm mgunet.predict_tta call (views + the group forwards + merge) | forward_ms: median of model(images) at the
  same B | ratio = tta_ms / forward_ms.

Each time is the median over `reps` calls, each call timed between HIP events and synchronised.  Prints one JSON line per case.  Run
under `rocprofv3 --kernel-trace --stats -- python tools/tta_bench.py` for the views and merge kernels' own times
(tta_views_kernel, tta_merge_kernel); `--bytes` prints the bytes each of them moves per case instead of timing anything."""
import argparse
import json

from benchkit import timed_each  # first: benchkit sets the import path
import torch

import mgunet
from mgunet import tta

CFG = (3, 2, 32, 4)
WARMUP = 3


def kernel_bytes(B, H, W, name, Cin=CFG[0], C=CFG[1]):
    """Compulsory bytes of the views kernel (read the image once per view, write every view but the lone identity) and of the merge
    kernel (read K * B * H * W * C logits, write probs, labels, confidence)."""
    views, groups = tta.view_table(name, H, W)
    K = len(views)
    vw = sum(len(g) for _, _, g in groups if g != [(0, 0)])
    return {"views_bytes": 2 * vw * B * Cin * H * W * 4, "merge_bytes": K * B * H * W * C * 4 + B * H * W * (C * 4 + 8 + 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--bytes", action="store_true", help="print the kernels' compulsory bytes per case and exit (no GPU)")
    args = ap.parse_args()
    H = W = args.size
    batches = [int(b) for b in args.batches.split(",")]
    if args.bytes:
        for B in batches:
            for name in ("none", "hflip", "d4"):
                print(json.dumps({"what": "tta_bytes", "B": B, "H": H, "W": W, "transforms": name, **kernel_bytes(B, H, W, name)}))
        return
    dev = torch.device("cuda:0")
    for dtype in (torch.float32, torch.bfloat16):
        model = mgunet.UNet(*CFG, compute_dtype=dtype).to(dev).eval()
        for B in batches:
            x = torch.randn((B, CFG[0], H, W), generator=torch.Generator().manual_seed(B)).to(dev)
            with torch.no_grad():
                fwd = timed_each(lambda: model(x), args.reps, WARMUP)
            for name in ("none", "hflip", "d4"):
                t = timed_each(lambda: tta.predict_tta(model, x, name), args.reps, WARMUP)
                print(json.dumps({"what": "tta", "dtype": str(dtype).split(".")[-1], "B": B, "H": H, "W": W, "transforms": name,
                                  "views": len(tta.TRANSFORMS[name]), "tta_ms": round(t, 3), "forward_ms": round(fwd, 3),
                                  "ratio": round(t / fwd, 3), **kernel_bytes(B, H, W, name)}), flush=True)
            del x
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
