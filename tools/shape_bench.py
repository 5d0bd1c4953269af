"""Object shape analysis at 8 x 512^2, one process, one GPU: mgunet.object_shapes (moments, finish and thin-object launches) against the dense
route it replaces for EllipticalShapeLoss -- ObjectTable.masks(), torch.stack, mgu_elliptical_shape_loss_masks.

    python tools/shape_bench.py --case scenes|one|many|full [--iters 20]

  scenes  eight scenes of 40 overlapping ellipses plus salt noise (tools/make_shape_golden.py's generator, seeds 7..14): object_shapes
          on every object and on the table labelled with min_area=10 (about 240 objects, all analysed), and the dense route on the
          latter (host clock around a synchronise: masks() reads the counts on the host)
  one     a single ellipse in the first image: 1 object
  many    250 squares of 5 x 5 pixels per image: 2 000 objects
  full    every image all foreground: 8 image-sized objects, every wave adding to the same 12 sums

Prints one JSON line per measurement (HIP events, the stream parked behind a spin kernel).  Every case runs object_shapes the same
number of times, so under `rocprofv3 --kernel-trace --stats -- python tools/shape_bench.py --case X` the launch counts of
moments_init_kernel, moments_kernel, shapes_kernel, residual_kernel and residual_finish_kernel are comparable between the cases (profiles/shapes_kernel_times.txt)."""
import argparse
import time

from benchkit import emit, timed  # first: benchkit sets the import path
import numpy as np
import torch

import mgunet
from make_shape_golden import ellipse, scene

B, H, W = 8, 512, 512
WARMUP = 5

def maps_of(case):
    m = np.zeros((B, H, W), np.int64)
    if case == "scenes":
        m[:] = np.stack([scene(seed) for seed in range(7, 7 + B)])
    elif case == "one":
        m[0] = ellipse(H, W, 250, 260, 20, 28, 0.3)
    elif case == "many":
        for k in range(250):
            y, x = 8 + 30 * (k // 16), 8 + 30 * (k % 16)
            m[:, y:y + 5, x:x + 5] = 1
    elif case == "full":
        m[:] = 1
    return m


def shapes_us(table, iters):
    return round(timed(lambda: mgunet.object_shapes(table), iters, WARMUP) * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=("scenes", "one", "many", "full"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cmap = torch.from_numpy(maps_of(a.case)).to(dev)
    table = mgunet.connected_components(cmap)
    sh = mgunet.object_shapes(table)
    emit(what="object_shapes", case=a.case, B=B, H=H, W=W, objects=table.area.numel(), analysed=int(sh.valid.sum()),
         largest_area=int(table.area.max()), object_shapes_us=shapes_us(table, a.iters), loss=float(sh.loss()))
    if a.case != "scenes":
        return
    t10 = mgunet.connected_components(cmap, min_area=10)
    sh10 = mgunet.object_shapes(t10)
    loss_fn = mgunet.EllipticalShapeLoss()
    stats_us = round(timed(lambda: mgunet.objects._stats(t10.labels, cmap, 0, B, H, W, 0, t10.offsets, t10.area.numel(), t10.class_id, t10.bbox,
                                                         t10.area, t10.sums), a.iters, WARMUP) * 1e3, 1)
    new_loss_us = round(timed(lambda: mgunet.object_shapes(t10).loss(), a.iters, WARMUP) * 1e3, 1)

    def dense():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loss_fn(None, t10.masks())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6, float(out)
    dense()
    runs = [dense() for _ in range(5)]
    dense_us = float(np.median([r[0] for r in runs]))
    emit(what="object_shapes_vs_dense", case="scenes min_area=10", objects=t10.area.numel(), analysed=int(sh10.valid.sum()),
         object_shapes_us=shapes_us(t10, a.iters), object_shapes_and_loss_us=new_loss_us, object_stats_us=stats_us,
         dense_masks_stack_loss_us=round(dense_us, 1), dense_over_new=round(dense_us / new_loss_us, 1), loss_new=float(sh10.loss()),
         loss_dense=runs[0][1], dense_mask_bytes=2 * t10.area.numel() * H * W)


if __name__ == "__main__":
    main()
