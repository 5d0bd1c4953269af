"""Object splitting at the flagship batch, one process, one GPU: B = 8 images of 512 x 512.

  scene      overlapping filled ellipses (clusters of two to four fruits), labelled by mgunet.connected_components
  worst      one full-image component pierced by a lattice of single background pixels: about a thousand seeds per image, every
             foreground pixel scans all of them (the pixels x seeds cost of the assignment)

For each: the device time of mgu_distance_transform alone and of mgu_split_objects on the label map (after labelling; HIP events
around calls queued behind a parked stream, so they time the GPU and not the host's launch rate), with the object counts before and
after.  For the scene also the host composition the call replaces: the label map copied to the host, scipy's
distance_transform_edt per object, the numpy oracle's split (tests/split_objects_oracle.py) on those distances and the copy back,
wall clock, once; the device result must equal it.  Prints one JSON line per measurement.  --quick: fewer iterations, no host run."""
import argparse
import functools
import time

import benchkit
import numpy as np
import torch
from benchkit import ellipse_scene, emit

import mgunet
from mgunet import objects

timed = functools.partial(benchkit.timed, warmup=3)


def pierced_scene(B, H, W, pitch=16):
    out = np.ones((B, H, W), np.int64)
    out[:, pitch // 2::pitch, pitch // 2::pitch] = 0
    return out


def host_split(labels_dev, r, r2):
    """The composition the device call replaces; returns (labels int32 on the device, seconds)."""
    from scipy import ndimage
    import split_objects_oracle as S
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab = labels_dev.cpu().numpy()
    res = []
    for m in lab:
        dist = np.zeros(m.shape, np.int64)
        for k in range(1, int(m.max()) + 1):
            mask = m == k
            dist[mask] = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64)[mask]
        res.append(S.split(m, r, r2, dist=dist.astype(np.int32))["labels"])
    out = torch.from_numpy(np.stack(res)).to(labels_dev.device)
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--min-distance", type=int, default=5)
    ap.add_argument("--min-radius", type=float, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = 8, 512, 512
    iters = 3 if args.quick else 20
    params = objects._split_params(args.min_distance, args.min_radius, 0)
    for tag, cmap in (("scene", ellipse_scene(B, H, W, 1)), ("worst", pierced_scene(B, H, W))):
        table = mgunet.connected_components(torch.from_numpy(cmap).to(dev))
        lab = table.labels
        out = torch.empty_like(lab)
        seeds = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
        counts = torch.empty(B, device=dev, dtype=torch.int64)
        offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
        run = lambda: objects._split(lab, B, H, W, params, out, counts, offsets, None, seeds)  # noqa: E731
        run()
        emit(what="workload", workload=tag, B=B, H=H, W=W, min_distance=params[0], min_radius_sq=params[1],
             foreground=round(float((lab > 0).float().mean()), 3), components=int(table.offsets[B]), seeds=int(seeds.sum()),
             objects=int(offsets[B]))
        emit(what="distance_transform", workload=tag, us=round(timed(lambda: mgunet.distance_transform(lab), iters) * 1e3, 1))
        emit(what="split_objects", workload=tag, us=round(timed(run, iters) * 1e3, 1))
        if tag == "scene" and not args.quick:
            ref, sec = host_split(lab, params[0], params[1])
            emit(what="host_composition", workload=tag, us=round(sec * 1e6, 1), same_labels=bool(torch.equal(ref, out)))


if __name__ == "__main__":
    main()
