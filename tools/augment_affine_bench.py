"""Scale / crop / colour augmentation (csrc/augment_affine.hip) at the flagship batch, one process, one GPU: 8 x 512 x 512 x 3 uint8
images and their uint8 masks -> the normalised fp32 (8, 3, 512, 512) batch and the int64 masks, through mgu_augment_affine_color with
a device-resident parameter table (what RandomAffineColor uploads per call).

Rows, each the device time of the call as the median of --runs timed loops of 20 calls with their spread (HIP events around calls
queued behind a parked stream: the GPU's time, not the host's launch rate):
  (a) copy        a device copy of the same output bytes (fp32 batch + int64 masks): what writing the result costs at the least
  (b) geometry    15 degrees, zoom 1, colour identity (no luma pass), on a scene and on a uniform image
  (c) colour      geometric identity, brightness / contrast / saturation / hue all off their neutral values (luma pass + main kernel)
  (d) both        15 degrees with the colour of (c) at zoom 0.5, 1 and 2, on a scene and on a uniform image; the split into the luma
                  and the main kernel from the context's profiling records of separate, synchronised calls
  (e) flip_rotate RandomFlipRotate's kernel (NEAREST, fp32 in, fp32 out) on the same batch, already normalised: the stage this adds to
  (f) torch       the same augmentation composed from torch on the device: F.affine_grid + F.grid_sample (bilinear image, nearest
                  mask), the luma mean, the colour matrix, clamp, /255, normalise; with the number of device ops it dispatches (each
                  at least one launch) and its largest difference from the kernel's output
One JSON line per measurement.  --quick: fewer iterations."""
import argparse
import ctypes as C

from benchkit import ellipse_scene, emit, median_spread  # first: benchkit sets the import path
import numpy as np
import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

import mgunet
from mgunet import _lib

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
COLOUR = (1.15, 0.85, 1.2, 0.015)


def sources(B, H, W, dev):
    """scene: fruit-coloured ellipses on a textured background, with its class map as the mask; uniform: one colour, one class"""
    rng = np.random.RandomState(0)
    g = ellipse_scene(B, H, W, 1)
    base = np.where(g[..., None] == 1, np.asarray([230, 150, 40]), np.asarray([60, 110, 50])).astype(np.float32)
    img = np.clip(base + rng.normal(0, 18, base.shape), 0, 255).astype(np.uint8)
    uni = np.empty_like(img)
    uni[:] = (90, 120, 60)
    to = lambda a: torch.from_numpy(a).to(dev)
    return {"scene": (to(img), to(g.astype(np.uint8))), "uniform": (to(uni), to(np.zeros_like(g, np.uint8)))}


def table(B, angle, zoom, colour, hw, dev):
    A, k = mgunet.color_matrix_q12(*colour) if colour else mgunet.color_matrix_q12()
    rows = [mgunet.affine_fixed(b % 2, angle if b % 2 else -angle, zoom, 1.0, 0.5, -0.5, hw, hw) + A + (k,) for b in range(B)]
    return torch.tensor(rows, dtype=torch.int32), k != 0


class OpCounter(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if not any(w in func.name() for w in ("view", "permute", "expand", "unsqueeze", "select", "reshape")):      # no kernel of their own
            self.n += 1
        return out


def torch_stage(img, mask, tab, H, W):
    """the composition a user would write on the device, from the same integer table"""
    B, Hs, Ws, _ = img.shape
    t = tab.to(torch.float64) / 65536.0
    a0, a1, a2, a3, a4, a5 = (t[:, i] for i in range(6))
    theta = torch.stack([torch.stack([a0 * W / Ws, a1 * H / Ws, (2.0 / Ws) * (a2 + a0 * (W / 2 - 0.5) + a1 * (H / 2 - 0.5) + 0.5) - 1.0], 1),
                         torch.stack([a3 * W / Hs, a4 * H / Hs, (2.0 / Hs) * (a5 + a3 * (W / 2 - 0.5) + a4 * (H / 2 - 0.5) + 0.5) - 1.0], 1)], 1).float()
    A = (tab[:, 6:15].float() / 4096.0).reshape(B, 3, 3)
    k = tab[:, 15].float() / 4096.0
    mean, std = (torch.tensor(v, device=img.device).reshape(1, 3, 1, 1) for v in (MEAN, STD))
    luma = torch.tensor([77.0, 150.0, 29.0], device=img.device).reshape(1, 3, 1, 1) / 256.0

    def run():
        x = img.permute(0, 3, 1, 2).float()
        grid = F.affine_grid(theta, (B, 3, H, W), align_corners=False)
        v = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        m = F.grid_sample(mask[:, None].float() + 100.0, grid, mode="nearest", padding_mode="zeros", align_corners=False)[:, 0].long() - 100
        mu = (x * luma).sum(1).mean((1, 2))
        y = torch.einsum("bij,bjhw->bihw", A, v) + (k * mu).reshape(B, 1, 1, 1)
        return (y.clamp(0.0, 255.0) / 255.0 - mean) / std, torch.where(m >= 0, m.clamp_max(1), m)
    return run


def stage_split(ctx, run, reps):
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
    return {k.replace("augment ", ""): round(float(np.median(v)), 1) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = _lib.context(dev)
    B, H, W = 8, 512, 512
    iters, runs = (3, 2) if args.quick else (20, args.runs)
    emit(what="setup", luma_tile=int(_lib.lib().mgu_augment_luma_tile()), iters=iters, loops=runs, B=B, H=H, W=W, colour=COLOUR)
    src = sources(B, H, W, dev)
    out = torch.empty((B, 3, H, W), device=dev)
    mout = torch.empty((B, H, W), device=dev, dtype=torch.int64)
    so = (C.c_int64 * 4)(*out.stride())
    mean, std, fill = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD), (C.c_uint8 * 3)(0, 0, 0)

    def stage(img, mask, tab_dev, need_mean):
        def run():
            _lib.call("mgu_augment_affine_color", dev, img, B, H, W, 0, mask, 2, out, H, W, so, mean, std, fill, mout, -100, tab_dev, int(need_mean))
        return run

    out2, mout2 = torch.empty_like(out), torch.empty_like(mout)

    def copy():
        out2.copy_(out)
        mout2.copy_(mout)

    stage(*src["scene"], table(B, 15.0, 1.0, None, (H, W), dev)[0].to(dev), False)()
    base, blo, bhi = median_spread(copy, iters, runs)
    emit(what="device", row="a copy", bytes=out.numel() * 4 + mout.numel() * 8, us={"median": base, "min": blo, "max": bhi})
    rows = [("b geometry", "scene", 15.0, 1.0, None), ("b geometry", "uniform", 15.0, 1.0, None), ("c colour", "scene", 0.0, 1.0, COLOUR),
            ("d both zoom 0.5", "scene", 15.0, 0.5, COLOUR), ("d both zoom 1", "scene", 15.0, 1.0, COLOUR), ("d both zoom 2", "scene", 15.0, 2.0, COLOUR),
            ("d both zoom 1", "uniform", 15.0, 1.0, COLOUR)]
    ours = {}
    for name, which, angle, zoom, colour in rows:
        tab, need_mean = table(B, angle, zoom, colour, (H, W), dev)
        run = stage(*src[which], tab.to(dev), need_mean)
        med, lo, hi = median_spread(run, iters, runs)
        ours[(name, which)] = med
        emit(what="device", row=name, source=which, us={"median": med, "min": lo, "max": hi}, over_copy=round(med / base, 2),
             stages_us=stage_split(ctx, run, 5))
    # (e) the NEAREST flip / rotation of the already normalised batch
    x = torch.randn((B, 3, H, W), device=dev)
    y = src["scene"][1].long()
    fr = mgunet.RandomFlipRotate(mask_fill=-100)
    ptab = fr.draw(B, W, H, generator=torch.Generator().manual_seed(0)).to(dev)
    si = (C.c_int64 * 4)(*x.stride())
    ffill = (C.c_float * 3)(*fr.fill)

    def flip_rotate():
        _lib.call("mgu_augment_flip_rotate", dev, x, out, B, 3, H, W, si, so, ffill, y, mout, -100, ptab)

    med, lo, hi = median_spread(flip_rotate, iters, runs)
    emit(what="device", row="e flip_rotate", us={"median": med, "min": lo, "max": hi}, over_copy=round(med / base, 2))
    # (f) the torch composition of "d both zoom 1" on the scene
    tab, _ = table(B, 15.0, 1.0, COLOUR, (H, W), dev)
    img, mask = src["scene"]
    stage(img, mask, tab.to(dev), True)()
    composed = torch_stage(img, mask, tab.to(dev), H, W)
    with OpCounter() as oc:
        ty, tm = composed()
    emit(what="torch_agreement", max_abs_diff=round(float((ty - out).abs().max()), 4), median_abs_diff=round(float((ty - out).abs().median()), 6),
         mask_agreement=round(float((tm == mout).float().mean()), 5), note="float32 bilinear with zero padding against 8-bit fractions and integer colour")
    tmed, tlo, thi = median_spread(composed, 3 if args.quick else 10, runs, warmup=1)
    emit(what="torch_composition", row="f torch", device_ops=oc.n, us={"median": tmed, "min": tlo, "max": thi},
         torch_over_stage=round(tmed / ours[("d both zoom 1", "scene")], 1))


if __name__ == "__main__":
    main()
