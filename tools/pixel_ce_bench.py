"""Pixel cross-entropy (csrc/pixel_ce.hip) at the flagship batch, one process, one GPU: value + gradient into the trainer's
pitch-padded dlogits at 8 x 512 x 512, C = 2 and C = 4, on the logits of an overlapping-ellipse scene (benchkit.ellipse_scene,
about 10-20 % foreground) plus unit noise, stored NHWC as the network leaves them.

Rows, each the device time of the call as the median of --runs timed loops of 20 calls with their spread (HIP events around calls
queued behind a parked stream: the GPU's time, not the host's launch rate):
  (a) ce             mgu_cross_entropy, the trainer's plain kernel: the yardstick
  (b) weights_smooth mgu_pixel_ce_backward with class weights and label_smoothing 0.1
  (c) focal          ... with focal_gamma 2
  (d) mined          (b) with keep_fraction 0.25, over the batch and per image, with the split into select / sums / gradient from the
                     context's profiling records of separate, synchronised calls (event pairs per launch: their sum exceeds the
                     queued time by the gaps)
  (e) all_equal      (d) over the batch with all logits equal: one tie over the group, every key in one bin per pass
  (f) torch          what (d) replaces on the device: F.cross_entropy(weight, label_smoothing, reduction="none"), torch.topk over the
                     batch or per image, the kept losses over the kept weights, autograd backward
Expected: (b) and (c) within what one more read of the logits explains over (a); (d) below (f).  One JSON line per measurement.
--quick: fewer iterations."""
import argparse

from benchkit import ellipse_scene, emit, median_spread  # first: benchkit sets the import path
import numpy as np
import torch
import torch.nn.functional as F

from mgunet import _lib

KEEP, EPS, GAMMA = 0.25, 0.1, 2.0


def scene(B, H, W, C, seed, dev, equal=False):
    """(logits (B, C, H, W) view of NHWC fp32 storage, labels int64 (B, H, W))"""
    rng = np.random.RandomState(seed)
    g = ellipse_scene(B, H, W, seed)
    if C > 2:
        g *= np.kron(rng.randint(1, C, (B, H // 64 + 1, W // 64 + 1)), np.ones((64, 64), np.int64))[:, :H, :W]
    lg = np.zeros((B, H, W, C), np.float32) if equal else (3.0 * np.eye(C, dtype=np.float32)[g] + rng.standard_normal((B, H, W, C)).astype(np.float32))
    return torch.from_numpy(lg).to(dev).permute(0, 3, 1, 2), torch.from_numpy(g).to(dev)


def torch_mined(logits, labels, weight, per_image):
    """the yardstick composition, no ignore_index: differentiable w.r.t. logits"""
    B = logits.shape[0]
    l = F.cross_entropy(logits, labels, weight=weight, label_smoothing=EPS, reduction="none").reshape(B, -1)
    wy = weight[labels].reshape(B, -1)
    if not per_image:
        l, wy = l.reshape(1, -1), wy.reshape(1, -1)
    k = int(np.ceil(KEEP * l.shape[1]))
    top, idx = torch.topk(l, k, dim=1)
    return top.sum() / wy.gather(1, idx).sum()


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
    return {k.replace("pixel_ce ", ""): round(float(np.median(v)), 1) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = _lib.context(dev)
    B, H, W = 8, 512, 512
    iters, runs = (3, 2) if args.quick else (20, args.runs)
    emit(what="setup", tile=int(_lib.lib().mgu_pixel_ce_tile()), iters=iters, loops=runs, B=B, H=H, W=W, keep_fraction=KEEP,
         label_smoothing=EPS, focal_gamma=GAMMA)
    for C in (2, 4):
        lg, y = scene(B, H, W, C, 1, dev)
        eq, _ = scene(B, H, W, C, 1, dev, equal=True)
        weight = torch.tensor([0.5, 2.0, 1.25, 0.75][:C], device=dev)
        ldd, HW = (C + 3) // 4 * 4, H * W
        dlogits = torch.zeros((B * HW, ldd), device=dev)
        loss = torch.zeros(1, device=dev)

        def ce():
            _lib.call("mgu_cross_entropy", dev, lg.permute(0, 2, 3, 1), y, B * HW, C, 1.0 / (B * HW), dlogits, loss)

        def pixel_ce(src, w, eps, gamma, keep, per_image):
            def run():
                _lib.call("mgu_pixel_ce_backward", dev, src.permute(0, 2, 3, 1), y, B, HW, C, HW * C, 1, C, w, eps, gamma, keep, 0, int(per_image),
                          -100, 1.0, None, dlogits, HW * ldd, 1, ldd, 0, ldd, loss)
            return run

        assert lg.permute(0, 2, 3, 1).is_contiguous()
        base, blo, bhi = median_spread(ce, iters, runs)
        emit(what="device", row="a ce", C=C, loss=round(float(loss), 6), us={"median": base, "min": blo, "max": bhi})
        rows = [("b weights_smooth", lg, weight, EPS, 0.0, 1.0, False), ("c focal", lg, weight, 0.0, GAMMA, 1.0, False),
                ("d mined batch", lg, weight, EPS, 0.0, KEEP, False), ("d mined per_image", lg, weight, EPS, 0.0, KEEP, True),
                ("e all_equal mined batch", eq, weight, EPS, 0.0, KEEP, False)]
        mined = {}
        for name, src, w, eps, gamma, keep, per_image in rows:
            run = pixel_ce(src, w, eps, gamma, keep, per_image)
            med, lo, hi = median_spread(run, iters, runs)
            mined[name] = (med, float(loss))
            emit(what="device", row=name, C=C, loss=round(float(loss), 6), us={"median": med, "min": lo, "max": hi},
                 over_ce=round(med / base, 2), stages_us=stage_split(ctx, run, 5))
        for per_image in (False, True):
            leaf = lg.detach().contiguous().requires_grad_(True)

            def composed():
                leaf.grad = None
                torch_mined(leaf, y, weight, per_image).backward()

            composed()
            ref = float(torch_mined(leaf, y, weight, per_image).detach())
            tmed, tlo, thi = median_spread(composed, 3 if args.quick else 10, runs, warmup=1)
            med, got = mined["d mined per_image" if per_image else "d mined batch"]
            emit(what="torch_composition", row="f torch", C=C, per_image=per_image, loss=round(ref, 6), us={"median": tmed, "min": tlo, "max": thi},
                 torch_over_mined=round(tmed / med, 1))
            assert abs(ref - got) <= 1e-4 * max(1.0, abs(ref)), (ref, got)


if __name__ == "__main__":
    main()
