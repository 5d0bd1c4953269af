"""Superpixel graphs at the flagship batch, one process, one GPU: B = 8 photographs of 512 x 512 x 3, step 16 (1024 centres per
image), 10 SLIC passes, min_area 64, 2 merge rounds.

  scene      overlapping ellipses of fruit colour on a leaf-green ground with Gaussian pixel noise (sigma 6)
  uniform    one grey level everywhere: every distance ties, and every pixel of a cell adds to the same accumulators

For each: the device time of the five stages on their own -- slic_labels, connect_regions, region_adjacency, region_features and
region_pool (32 channels) -- and of the whole superpixel_graph, as the median (min, max) of 5 loops of 20 calls between HIP events
behind a parked stream, through the public functions (their output allocations included); next to a device copy of the images' bytes.
For the scene also the numpy oracle (tests/superpixels_oracle.py) on the host for the identical result, wall clock, once; the device
result must equal it.  Prints one JSON line per measurement.  --quick: fewer iterations, no host run."""
import argparse
import time

import benchkit
import numpy as np
import torch
from benchkit import ellipse_scene, emit, median_spread

import mgunet


def photo_scene(B, H, W, seed=1, sigma=6.0):
    cmap = ellipse_scene(B, H, W, seed)
    rng = np.random.default_rng(seed)
    img = np.where(cmap[..., None] > 0, np.array([230.0, 170.0, 40.0]), np.array([40.0, 90.0, 35.0]))
    return np.clip(np.rint(img + rng.normal(0.0, sigma, img.shape)), 0, 255).astype(np.uint8)


def host_graph(img, S, mq, T, min_area, rounds, ncap):
    import superpixels_oracle as SO
    t0 = time.perf_counter()
    raw, _ = SO.slic(img, S, mq, T)
    labels, counts, offsets = SO.connect(raw, min_area, rounds)
    rowptr, col, border, _ = SO.adjacency(labels, offsets, ncap)
    feat, _ = SO.features(img, labels, offsets, ncap)
    return (labels, offsets, rowptr, col, border, feat), time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W, S, T, D = 8, 512, 512, 16, 10, 32
    min_area, rounds = S * S // 4, 2
    iters, runs = (3, 2) if args.quick else (20, 5)
    stat = lambda fn: dict(zip(("us", "us_min", "us_max"), median_spread(fn, iters, runs)))  # noqa: E731
    fmap = torch.randn((B, H, W, D), device=dev).permute(0, 3, 1, 2)
    for tag, host in (("scene", photo_scene(B, H, W)), ("uniform", np.full((B, H, W, 3), 120, np.uint8))):
        img = torch.from_numpy(host).to(dev)
        raw = mgunet.slic_labels(img, step=S, iterations=T)
        labels, counts, offsets = mgunet.connect_regions(raw, min_area, rounds)
        g = mgunet.superpixel_graph(img, step=S, iterations=T).check()
        ncap = g.node_capacity
        emit(what="workload", workload=tag, B=B, H=H, W=W, step=S, passes=T, min_area=min_area, rounds=rounds, centres=int(B * (H // S) * (W // S)),
             components=int(mgunet.connect_regions(raw, 0, 0)[2][B]), regions=int(offsets[B]), directed_edges=int(g.rowptr[-1]),
             node_capacity=ncap, edge_capacity=g.edge_capacity)
        emit(what="device_copy_of_the_images", workload=tag, bytes=img.numel(), **stat(lambda: img.clone()))
        emit(what="slic_labels", workload=tag, **stat(lambda: mgunet.slic_labels(img, step=S, iterations=T)))
        emit(what="slic_labels_one_pass", workload=tag, **stat(lambda: mgunet.slic_labels(img, step=S, iterations=1)))
        emit(what="connect_regions", workload=tag, **stat(lambda: mgunet.connect_regions(raw, min_area, rounds)))
        emit(what="region_adjacency", workload=tag, **stat(lambda: mgunet.region_adjacency(labels, offsets, ncap)))
        emit(what="region_features", workload=tag, **stat(lambda: mgunet.region_features(img, labels, offsets, ncap)))
        emit(what="region_pool", workload=tag, channels=D, **stat(lambda: mgunet.region_pool(fmap, labels, offsets, ncap)))
        emit(what="superpixel_graph", workload=tag, **stat(lambda: mgunet.superpixel_graph(img, step=S, iterations=T)))
        if tag == "scene" and not args.quick:
            ref, sec = host_graph(host, S, 40, T, min_area, rounds, ncap)
            E = int(ref[2][-1])
            same = (np.array_equal(g.labels.cpu().numpy(), ref[0]) and np.array_equal(g.offsets.cpu().numpy(), ref[1]) and
                    np.array_equal(g.rowptr.cpu().numpy(), ref[2]) and np.array_equal(g.col[:E].cpu().numpy(), ref[3]) and
                    np.array_equal(g.border[:E].cpu().numpy(), ref[4]) and np.array_equal(g.features.cpu().numpy(), ref[5]))
            emit(what="numpy_oracle_on_the_host", workload=tag, us=round(sec * 1e6, 1), same_result=bool(same))


if __name__ == "__main__":
    main()
