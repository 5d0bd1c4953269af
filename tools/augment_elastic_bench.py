"""Elastic deformation in the scale / crop / colour pass (csrc/augment_elastic.hip) at the flagship batch, one process, one GPU:
8 x 512 x 512 x 3 uint8 images with their uint8 masks and int32 instance maps -> the normalised fp32 (8, 3, 512, 512) batch, the int64
masks and the int32 instance maps, through mgu_augment_elastic_color with device-resident parameter and control tables (15 degrees,
zoom 1, the colour of tools/augment_affine_bench.py, sigma 10 pixels).

Rows, each the device time of the call as the median of --runs timed loops of 20 calls with their spread (HIP events around calls
queued behind a parked stream: the GPU's time, not the host's launch rate), for 6 x 6 and 32 x 32 control nodes:
  (a) copy           a device copy of the same output bytes (fp32 batch + int64 masks + int32 labels)
  (b) affine         mgu_augment_affine_color on the same parameter table (images + masks): the unchanged kernel, the yardstick
  (c) no field       the new entry without control nodes: images + masks, and images + masks + labels (what the labels cost)
  (d) elastic        the new entry with the field: images + masks, and images + masks + labels; elastic_over_affine is (d, images + masks)
                     over (b), the same outputs from the same table; the split into the luma and the main kernel from the context's
                     profiling records of separate, synchronised calls
  (e) field          mgu_elastic_field alone (int32 (8, 2, 512, 512))
  (f) torch          the same stage composed from torch on the device: F.interpolate(bicubic) of the coarse field (the spline's values at
                     the inner nodes), F.affine_grid, the add, F.grid_sample (bilinear image, nearest mask and labels), the luma mean,
                     the colour matrix, clamp, /255, normalise; with the number of device ops it dispatches and its difference from the
                     kernel's output in normalised units (bicubic convolution follows the cubic B-spline to a fraction of a pixel, not
                     exactly: the two fields differ by construction, and with them the pixels on edges)
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
COLOUR = (1.15, 0.85, 1.2, 0.015)      # brightness, contrast, saturation, hue of tools/augment_affine_bench.py
SIGMA = 10.0


def scene(B, H, W, dev):
    """fruit-coloured ellipses on a textured background, with its class map as the mask (the scene of tools/augment_affine_bench.py)"""
    rng = np.random.RandomState(0)
    g = ellipse_scene(B, H, W, 1)
    base = np.where(g[..., None] == 1, np.asarray([230, 150, 40]), np.asarray([60, 110, 50])).astype(np.float32)
    img = np.clip(base + rng.normal(0, 18, base.shape), 0, 255).astype(np.uint8)
    return torch.from_numpy(img).to(dev), torch.from_numpy(g.astype(np.uint8)).to(dev)


def table(B, angle, zoom, colour, hw):
    A, k = mgunet.color_matrix_q12(*colour)
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


def stage_split(ctx, run, reps):
    """median event-pair time per kernel family, microseconds, of separate synchronised calls"""
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


def control(tab, nodes, seed):
    g = torch.Generator().manual_seed(seed)
    gh, gw = nodes
    return torch.stack([mgunet.elastic_control(torch.randn(2 * gh * gw, dtype=torch.float64, generator=g).reshape(2, gh, gw).numpy(), SIGMA, row, nodes)
                        for row in tab.tolist()])


def torch_stage(img, mask, labels, tab, ctrl, H, W):
    """the composition a user would write on the device, from the same integer tables"""
    B, Hs, Ws, _ = img.shape
    t = tab.to(torch.float64) / 65536.0
    a0, a1, a2, a3, a4, a5 = (t[:, i] for i in range(6))
    theta = torch.stack([torch.stack([a0 * W / Ws, a1 * H / Ws, (2.0 / Ws) * (a2 + a0 * (W / 2 - 0.5) + a1 * (H / 2 - 0.5) + 0.5) - 1.0], 1),
                         torch.stack([a3 * W / Hs, a4 * H / Hs, (2.0 / Hs) * (a5 + a3 * (W / 2 - 0.5) + a4 * (H / 2 - 0.5) + 0.5) - 1.0], 1)], 1).float()
    A = (tab[:, 6:15].float() / 4096.0).reshape(B, 3, 3)
    k = tab[:, 15].float() / 4096.0
    mean, std = (torch.tensor(v, device=img.device).reshape(1, 3, 1, 1) for v in (MEAN, STD))
    luma = torch.tensor([77.0, 150.0, 29.0], device=img.device).reshape(1, 3, 1, 1) / 256.0
    # the B-spline surface AT the inner nodes is their (1, 4, 1) / 6 average in each direction; bicubic interpolation through those values
    # follows the surface to a fraction of a pixel (through the raw nodes it would overshoot it by the nodes' own spread)
    unit = torch.tensor([2.0 / Ws, 2.0 / Hs], device=img.device).reshape(1, 2, 1, 1) / 65536.0       # 16.16 source pixels -> grid_sample's units
    k1 = torch.tensor([1.0, 4.0, 1.0], device=img.device) / 6.0
    k2 = (k1[:, None] * k1[None, :]).reshape(1, 1, 3, 3).repeat(2, 1, 1, 1)

    def run():
        x = img.permute(0, 3, 1, 2).float()
        d = F.interpolate(F.conv2d(ctrl.float() * unit, k2, groups=2), size=(H, W), mode="bicubic", align_corners=True)
        grid = F.affine_grid(theta, (B, 3, H, W), align_corners=False) + d.permute(0, 2, 3, 1)
        v = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        m = F.grid_sample(mask[:, None].float() + 100.0, grid, mode="nearest", padding_mode="zeros", align_corners=False)[:, 0].long() - 100
        ids = F.grid_sample(labels[:, None].float(), grid, mode="nearest", padding_mode="zeros", align_corners=False)[:, 0].int()
        mu = (x * luma).sum(1).mean((1, 2))
        y = torch.einsum("bij,bjhw->bihw", A, v) + (k * mu).reshape(B, 1, 1, 1)
        return (y.clamp(0.0, 255.0) / 255.0 - mean) / std, torch.where(m >= 0, m.clamp_max(1), m), ids
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = _lib.context(dev)
    B, H, W = 8, 512, 512
    iters, runs = (3, 2) if args.quick else (20, args.runs)
    emit(what="setup", iters=iters, loops=runs, B=B, H=H, W=W, colour=COLOUR, sigma=SIGMA, angle=15.0, zoom=1.0)
    img, mask = scene(B, H, W, dev)
    # instance ids: the scene's class map cut into 64 x 64 blocks, ids of a dataset's own (sparse, above 2^24)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev) // 64, torch.arange(W, device=dev) // 64, indexing="ij")
    labels = (mask.int() * ((1 << 24) + 1 + yy * 8 + xx).int()).contiguous()
    out = torch.empty((B, 3, H, W), device=dev)
    mout = torch.empty((B, H, W), device=dev, dtype=torch.int64)
    lout = torch.empty((B, H, W), device=dev, dtype=torch.int32)
    so = (C.c_int64 * 4)(*out.stride())
    mean, std, fill = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD), (C.c_uint8 * 3)(0, 0, 0)
    tab, need_mean = table(B, 15.0, 1.0, COLOUR, (H, W))
    tab_dev = tab.to(dev)

    def affine():
        _lib.call("mgu_augment_affine_color", dev, img, B, H, W, 0, mask, 2, out, H, W, so, mean, std, fill, mout, -100, tab_dev, int(need_mean))

    def elastic(ctrl_dev, with_labels):
        gh, gw = (int(ctrl_dev.shape[2]), int(ctrl_dev.shape[3])) if ctrl_dev is not None else (0, 0)

        def run():
            _lib.call("mgu_augment_elastic_color", dev, img, B, H, W, 0, mask, 2, out, H, W, so, mean, std, fill, mout, -100, tab_dev, int(need_mean),
                      labels if with_labels else None, lout if with_labels else None, 0, ctrl_dev, gh, gw)
        return run

    out2, mout2, lout2 = torch.empty_like(out), torch.empty_like(mout), torch.empty_like(lout)

    def copy():
        out2.copy_(out)
        mout2.copy_(mout)
        lout2.copy_(lout)

    affine()
    base, blo, bhi = median_spread(copy, iters, runs)
    emit(what="device", row="a copy", bytes=out.numel() * 4 + mout.numel() * 8 + lout.numel() * 4, us={"median": base, "min": blo, "max": bhi})
    aff, lo, hi = median_spread(affine, iters, runs)
    emit(what="device", row="b affine", outputs="images + masks", us={"median": aff, "min": lo, "max": hi}, over_copy=round(aff / base, 2),
         stages_us=stage_split(ctx, affine, 5))
    for with_labels in (False, True):
        med, lo, hi = median_spread(elastic(None, with_labels), iters, runs)
        emit(what="device", row="c no field", outputs="images + masks" + (" + labels" if with_labels else ""), us={"median": med, "min": lo, "max": hi},
             over_affine=round(med / aff, 2))
    for nodes in ((6, 6), (32, 32)):
        ctrl_dev = control(tab, nodes, 7).to(dev)
        for with_labels in (False, True):
            run = elastic(ctrl_dev, with_labels)
            el, lo, hi = median_spread(run, iters, runs)
            aff2 = median_spread(affine, iters, runs)[0]                       # the yardstick again, beside the row it is compared with
            emit(what="device", row="d elastic", nodes=list(nodes), outputs="images + masks" + (" + labels" if with_labels else ""),
                 us={"median": el, "min": lo, "max": hi}, affine_us=aff2, elastic_over_affine=round(el / aff2, 2), over_copy=round(el / base, 2),
                 stages_us=stage_split(ctx, run, 5))
        field = torch.empty((B, 2, H, W), device=dev, dtype=torch.int32)

        def field_alone():
            _lib.call("mgu_elastic_field", dev, ctrl_dev, B, nodes[0], nodes[1], H, W, field)

        med, lo, hi = median_spread(field_alone, iters, runs)
        emit(what="device", row="e field", nodes=list(nodes), bytes=field.numel() * 4, us={"median": med, "min": lo, "max": hi},
             max_abs_field_px=round(float(field.abs().max()) / 65536.0, 2))
        # (f) the torch composition
        elastic(ctrl_dev, True)()
        composed = torch_stage(img, mask, labels, tab_dev, ctrl_dev, H, W)
        with OpCounter() as oc:
            ty, tm, tl = composed()
        emit(what="torch_agreement", nodes=list(nodes), max_abs_diff=round(float((ty - out).abs().max()), 4),
             median_abs_diff=round(float((ty - out).abs().median()), 6), mask_agreement=round(float((tm == mout).float().mean()), 5),
             label_agreement=round(float((tl == lout).float().mean()), 5),
             note="normalised units; bicubic convolution through the spline's node values against the cubic B-spline, float32 bilinear against 8-bit fractions; "
                  "labels above 2^24 pass through float32 in torch")
        tmed, tlo, thi = median_spread(composed, 3 if args.quick else 10, runs, warmup=1)
        emit(what="torch_composition", row="f torch", nodes=list(nodes), device_ops=oc.n, us={"median": tmed, "min": tlo, "max": thi},
             torch_over_stage=round(tmed / el, 1))


if __name__ == "__main__":
    main()
