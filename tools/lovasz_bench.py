"""Lovasz-Softmax loss at the flagship batch, one process, one GPU: value + gradient (mgu_lovasz_softmax_backward into the trainer's
pitch-padded dlogits) at 8 x 512 x 512 and 4 x 512 x 512, C = 2 and C = 4, over the batch and per image, on the logits of an
overlapping-ellipse scene (benchkit.ellipse_scene, about 10-20 % foreground) plus unit noise, stored NHWC as the network leaves them.

For each: the device time of the call as the median of --runs timed loops of 20 calls with their spread (HIP events around calls
queued behind a parked stream: the GPU's time, not the host's launch rate), its split into the sort (the passes of histogram, scan,
scatter), the scan (foreground count, its scan, the closed forms, the finishing kernel) and the final per-pixel pass from the
context's profiling records of separate, synchronised calls (event pairs per stage: their sum exceeds the queued time by the gaps),
and three yardsticks:
  (a) dice       mgu_dice_loss_backward on the same tensors: a loss that is one streaming pass
  (b) torch      the same loss composed of torch operators on the device, written for this tool: softmax, torch.sort(descending=True,
                 stable=True) per class, cumsum, the Jaccard increments by the closed forms in float64, autograd backward
  (c) step       bench.py --mode train's step time (--step-ms, from a run of bench.py in the same job; 4 x 512 x 512, C = 2): what
                 "ce+lovasz" adds to a step, as a fraction of it
Worst case: all logits equal, one tie over every segment, every key in one bin per pass.  MGU_LOVASZ_PASSES=3 in the environment
times the 10 + 10 + 11 split instead of 8 + 8 + 8 + 7 (the tool prints which one ran).  One JSON line per measurement.
--quick: fewer iterations, one size."""
import argparse
import os

from benchkit import ellipse_scene, emit, median_spread  # first: benchkit sets the import path
import numpy as np
import torch

from mgunet import _lib


def scene(B, H, W, C, seed, dev, equal=False):
    """(logits (B, C, H, W) view of NHWC fp32 storage, labels int64 (B, H, W))"""
    rng = np.random.RandomState(seed)
    g = ellipse_scene(B, H, W, seed)
    if C > 2:
        g *= np.kron(rng.randint(1, C, (B, H // 64 + 1, W // 64 + 1)), np.ones((64, 64), np.int64))[:, :H, :W]
    lg = np.zeros((B, H, W, C), np.float32) if equal else (3.0 * np.eye(C, dtype=np.float32)[g] + rng.standard_normal((B, H, W, C)).astype(np.float32))
    return torch.from_numpy(lg).to(dev).permute(0, 3, 1, 2), torch.from_numpy(g).to(dev)


def torch_lovasz(logits, labels, per_image):
    """the yardstick composition, classes="present", no ignore_index: differentiable w.r.t. logits"""
    B, C = logits.shape[:2]
    p = torch.softmax(logits, dim=1)
    groups = [(p[b:b + 1], labels[b:b + 1]) for b in range(B)] if per_image else [(p, labels)]
    total = 0.0
    for pg, yg in groups:
        terms = []
        for c in range(C):
            fg = (yg == c).reshape(-1)
            G = fg.sum()
            if int(G) == 0:
                continue
            pc = pg[:, c].reshape(-1)
            e = torch.where(fg, 1.0 - pc, pc)
            es, order = torch.sort(e, descending=True, stable=True)
            fs = fg[order]
            F = torch.cumsum(fs, 0).double()
            U = G.double() + torch.arange(1, len(e) + 1, device=e.device, dtype=torch.float64) - F
            g = torch.where(fs, 1.0 / U, (G.double() - F) / (U * (U - 1.0)).clamp_min(1.0))
            terms.append((es * g.float()).sum())
        if terms:
            total = total + sum(terms) / len(terms)
    return total / len(groups)


def stage_split(ctx, run, reps):
    """median microseconds per stage over `reps` synchronised calls, from the context's profiling records"""
    L = _lib.lib()
    out = {}
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        for _ in range(reps):
            run()
            torch.cuda.synchronize()
            for k in _lib.read_kernel_stats(ctx):
                out.setdefault(k["name"], []).append(k["ms"] * 1e3)
    finally:
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return {k.replace("lovasz ", ""): round(float(np.median(v)), 1) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=None, help="bench.py --mode train step time of the same job, for the share")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = _lib.context(dev)
    H = W = 512
    iters, runs = (3, 2) if args.quick else (20, args.runs)
    emit(what="setup", passes=3 if os.environ.get("MGU_LOVASZ_PASSES") == "3" else 4, tile=int(_lib.lib().mgu_lovasz_tile()), iters=iters, loops=runs)
    for B in ((8,) if args.quick else (8, 4)):
        for C in (2, 4):
            for workload in ("scene", "all_equal"):
                lg, y = scene(B, H, W, C, 1, dev, equal=workload == "all_equal")
                nhwc = lg.permute(0, 2, 3, 1)
                assert nhwc.is_contiguous()
                ldd, HW = (C + 3) // 4 * 4, H * W
                dlogits = torch.zeros((B * HW, ldd), device=dev)
                loss = torch.zeros(1, device=dev)

                def dice():
                    _lib.call("mgu_dice_loss_backward", dev, nhwc, y, B, HW, C, HW * C, 1, C, 1.0, 1.0, None, dlogits, HW * ldd, 1, ldd, 1, loss)

                dmed, dlo, dhi = median_spread(dice, iters, runs)
                for per_image in (False, True):
                    if workload == "all_equal" and per_image:
                        continue

                    def lovasz():
                        _lib.call("mgu_lovasz_softmax_backward", dev, nhwc, y, B, HW, C, HW * C, 1, C, 0, int(per_image), -100, 1.0, None,
                                  dlogits, HW * ldd, 1, ldd, 1, loss)

                    med, lo, hi = median_spread(lovasz, iters, runs)
                    rec = dict(what="device", workload=workload, B=B, C=C, H=H, W=W, per_image=per_image, loss=round(float(loss), 6),
                               lovasz_us={"median": med, "min": lo, "max": hi}, stages_us=stage_split(ctx, lovasz, 5),
                               dice_us={"median": dmed, "min": dlo, "max": dhi}, lovasz_over_dice=round(med / dmed, 1))
                    if args.step_ms:
                        rec["added_to_train_step"] = round(med / (args.step_ms * 1e3), 3) if (B, C) == (4, 2) else None   # bench.py trains 4 x 512 x 512, C = 2
                    emit(**rec)
                    if workload == "scene" and not args.quick:
                        leaf = lg.detach().contiguous().requires_grad_(True)

                        def composed():
                            leaf.grad = None
                            torch_lovasz(leaf, y, per_image).backward()

                        composed()
                        ref = float(torch_lovasz(leaf, y, per_image).detach())
                        tmed, tlo, thi = median_spread(composed, 3, 3, warmup=1)
                        emit(what="torch_composition", B=B, C=C, per_image=per_image, loss=round(ref, 6), torch_us={"median": tmed, "min": tlo, "max": thi},
                             torch_over_lovasz=round(tmed / med, 1))
                        assert abs(ref - float(loss)) <= 1e-4, (ref, float(loss))


if __name__ == "__main__":
    main()
