"""The border weight map at the flagship batch, one process, one GPU: B = 8 images of 512 x 512.

  ellipses_cc      overlapping filled ellipses (clusters of two to four fruits), labelled by mgunet.connected_components
  ellipses_split   the same, cut apart by mgunet.split_objects: touching instances, the case the map is for
  one_object       one disc per image: no second object, so every pixel walks its whole row (the known worst case)
  empty            no object at all: the same walk, with nothing to merge
  dense_grid       4 x 4 squares at pitch 16, 1024 objects per image

For each: the device time of mgu_border_weights writing the three distance maps and writing the weight map (medians of 5 loops of 20
calls with the spread; HIP events around calls queued behind a parked stream, so they time the GPU and not the host's launch rate),
of mgu_distance_transform on the same labels, and of a device copy of the three distance maps' bytes.  Then the host composition
the call replaces, wall clock, once: the label map copied to the host, scipy's distance_transform_edt per object, the two smallest
kept per pixel, the exponential, the copy back (dense_grid: one image only -- 1024 transforms); the device weights must agree.
Last, Trainer's step on UNet(3, 2, 32, 4) with the map (border_w0 = 10, labels from the masks) against the same step with ce_weight
only (border_w0 = 0: the calls of a build without the map).  Prints one JSON line per measurement.  --quick: fewer iterations, no
host run, no trainer."""
import argparse

import benchkit
import numpy as np
import torch
from benchkit import ellipse_scene, emit, median_spread

import mgunet
from mgunet import border

W0, SIGMA = 10.0, 5.0


def disc_scene(B, H, W, r=40):
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W), np.int64)
    for b in range(B):
        out[b][(ys - (100 + 40 * b)) ** 2 + (xs - (400 - 35 * b)) ** 2 <= r * r] = 1
    return out


def grid_scene(B, H, W, pitch=16, side=4):
    ys, xs = np.mgrid[0:H, 0:W]
    return np.broadcast_to(((ys % pitch < side) & (xs % pitch < side)).astype(np.int64), (B, H, W)).copy()


def host_weights(labels_dev, w0, sigma):
    """The composition the device call replaces; returns (weights fp32 on the device, seconds)."""
    import time

    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab = labels_dev.cpu().numpy()
    res = []
    for m in lab:
        d1, d2 = np.full(m.shape, np.inf), np.full(m.shape, np.inf)
        for k in np.unique(m[m != 0]):
            d = ndimage.distance_transform_edt(m != k)
            d2 = np.minimum(d2, np.maximum(d1, d))             # the two smallest so far: a sort of the stack, streamed
            d1 = np.minimum(d1, d)
        with np.errstate(invalid="ignore"):
            e = np.where(np.isinf(d2), 0.0, w0 * np.exp(-(d1 + d2) ** 2 / (2.0 * sigma * sigma)))
        res.append((1.0 + e).astype(np.float32))
    out = torch.from_numpy(np.stack(res)).to(labels_dev.device)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = 8, 512, 512
    iters, runs = (3, 2) if args.quick else (20, 5)
    ell = torch.from_numpy(ellipse_scene(B, H, W, 1)).to(dev)
    scenes = (("ellipses_cc", mgunet.connected_components(ell).labels), ("ellipses_split", mgunet.split_objects(ell).labels),
              ("one_object", mgunet.connected_components(torch.from_numpy(disc_scene(B, H, W)).to(dev)).labels),
              ("empty", torch.zeros((B, H, W), device=dev, dtype=torch.int32)),
              ("dense_grid", mgunet.connected_components(torch.from_numpy(grid_scene(B, H, W)).to(dev)).labels))
    dist = torch.empty((3, B, H, W), device=dev, dtype=torch.int32)
    copy = torch.empty_like(dist)
    weight = torch.empty((B, H, W), device=dev, dtype=torch.float32)
    for tag, lab in scenes:
        lab = lab.contiguous()
        only_d = lambda: border._run(lab, None, None, W0, SIGMA, 0, dist[0], dist[1], dist[2], None, None)  # noqa: E731
        only_w = lambda: border._run(lab, None, None, W0, SIGMA, 0, None, None, None, weight, None)  # noqa: E731
        only_d(), only_w()
        objs = [int(torch.unique(lab[b]).numel()) - int(bool((lab[b] == 0).any())) for b in range(B)]
        emit(what="workload", workload=tag, B=B, H=H, W=W, w0=W0, sigma=SIGMA, foreground=round(float((lab != 0).float().mean()), 3),
             objects=sum(objs), objects_per_image_max=max(objs), weight_max=round(float(weight.max()), 3))
        for what, fn in (("border_distances", only_d), ("border_weights", only_w), ("distance_transform", lambda: mgunet.distance_transform(lab)),
                         ("copy_12_bytes_per_pixel", lambda: copy.copy_(dist))):
            med, lo, hi = median_spread(fn, iters, runs)
            emit(what=what, workload=tag, us=med, min_us=lo, max_us=hi)
        if not args.quick:
            sub = lab[:1] if tag == "dense_grid" else lab
            ref, sec = host_weights(sub, W0, SIGMA)
            emit(what="host_composition", workload=tag, images=int(sub.shape[0]), us=round(sec * 1e6, 1),
                 max_abs_diff=float((ref - weight[:sub.shape[0]]).abs().max()))
    if args.quick:
        return
    # the trainer's step: the flagship network on the ellipse masks, class weights only against class weights + the border map
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    cw = torch.tensor([0.5, 2.0])
    for tag, kw in (("ce_weight_only", {}), ("border_map", {"border_w0": W0, "border_sigma": SIGMA}),
                    ("border_map_separate", {"border_w0": W0, "border_sigma": SIGMA, "border_separate": True})):
        tr = mgunet.Trainer(mgunet.UNet(3, 2, 32, 4).to(dev), lr=1e-3, weight_decay=1e-4, comm=None, ce_weight=cw, **kw)
        ms = sorted(benchkit.wall(lambda: tr.train_step(x, ell), 10, 3) for _ in range(5))
        emit(what="trainer_step", workload=tag, ms=round(ms[2], 3), min_ms=round(ms[0], 3), max_ms=round(ms[4], 3), loss=round(float(tr.train_step(x, ell)), 4))
        del tr
    tr = mgunet.Trainer(mgunet.UNet(3, 2, 32, 4).to(dev), comm=None, ce_weight=cw, border_w0=W0, border_sigma=SIGMA)
    ms = sorted(benchkit.wall(lambda: tr.train_step(x, ell, instances=scenes[1][1]), 10, 3) for _ in range(5))
    emit(what="trainer_step", workload="border_map_instances_given", ms=round(ms[2], 3), min_ms=round(ms[0], 3), max_ms=round(ms[4], 3))


if __name__ == "__main__":
    main()
