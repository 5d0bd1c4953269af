"""Instance evaluation at the flagship batch, one process, one GPU: B = 8 images of 512 x 512.

  scene      the overlapping ellipses of benchkit.ellipse_scene, split into objects, as the prediction; the same class map
             shifted by (3, 2) pixels with 1 % of its pixels cleared, split alike, as the ground truth
  worst      one full-image object on both sides: every pixel adds to ONE pair, the most contended counter there can be

For each: the device time of mgu_object_overlaps alone and of the whole device path -- overlaps + mgu_match_masks at the ten
thresholds 0.50:0.05:0.95 in score order + mgu_panoptic_totals -- on label maps and per-object arrays already on the device (HIP
events around calls queued behind a parked stream, so they time the GPU and not the host's launch rate).  For both also the host
composition the path replaces: both label maps copied to the host, np.unique over the pixel pairs, the Python greedy loop per
threshold and the panoptic count (tests/instances_oracle.py), wall clock, once; the device results must equal it bit for bit.
Prints one JSON line per measurement.  --quick: fewer iterations, no host run."""
import argparse
import functools
import time

import benchkit
import numpy as np
import torch
from benchkit import ellipse_scene, emit

import mgunet
from mgunet import _lib, instances

timed = functools.partial(benchkit.timed, warmup=3)


def host_composition(tg, tp, scores, thresholds, C):
    """What the device path replaces; returns (match_gt, match_iou, totals, pq words, pairs, seconds)."""
    import instances_oracle as IO
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gt, pr = tg.labels.cpu().numpy(), tp.labels.cpu().numpy()
    gcls, pcls, sc = tg.class_id.cpu().numpy(), tp.class_id.cpu().numpy(), scores.cpu().numpy()
    table, dense = {}, IO.dense

    def dense_once(g, p, b):   # np.unique over an image's pixel pairs runs once, whoever asks
        if b not in table:
            table[b] = dense(g, p, b)
        return table[b]

    IO.dense = dense_once
    try:
        mg, mi, totals = IO.match(gt, pr, gcls, pcls, list(thresholds), sc)
        words, _ = IO.panoptic(gt, pr, gcls, pcls, C)
    finally:
        IO.dense = dense
    pairs = sum(int(np.count_nonzero(m)) for m in table.values())
    return mg, mi, totals, words, pairs, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W, C = 8, 512, 512, 2
    iters = 3 if args.quick else 20
    th = instances.DEFAULT_THRESHOLDS
    thr = torch.from_numpy(th).to(dev)
    scene = ellipse_scene(B, H, W, 1)
    moved = np.roll(scene, (3, 2), (1, 2))
    moved[np.random.RandomState(2).rand(B, H, W) < 0.01] = 0
    ones = np.ones((B, H, W), np.int64)
    for tag, pr_map, gt_map, split in (("scene", scene, moved, True), ("worst", ones, ones, False)):
        make = mgunet.split_objects if split else mgunet.connected_components
        tp, tg = make(torch.from_numpy(pr_map).to(dev)), make(torch.from_numpy(gt_map).to(dev))
        n_gt, n_pred, n = tg.class_id.numel(), tp.class_id.numel(), B * H * W
        scores = torch.rand(n_pred, generator=torch.Generator().manual_seed(3)).to(dev)
        pairs = (torch.empty(n_pred + 1, device=dev, dtype=torch.int64), torch.empty(n, device=dev, dtype=torch.int64),
                 torch.empty(n, device=dev, dtype=torch.int64))
        status = torch.zeros(1, device=dev, dtype=torch.int32)
        mg = torch.full((th.size, n_pred), -1, device=dev, dtype=torch.int64)
        mi = torch.zeros((th.size, n_pred), device=dev, dtype=torch.float64)
        totals = torch.zeros((th.size, 3), device=dev, dtype=torch.int64)
        pq = torch.zeros((C, 4), device=dev, dtype=torch.int64)
        sides = instances._sides(pairs, tg.offsets, tg.class_id, tg.area, n_gt, tp.offsets, tp.class_id, tp.area, n_pred)

        def overlaps():
            instances._overlaps(tg.labels, tg.offsets, n_gt, tp.labels, tp.offsets, n_pred, B, H, W, *pairs, status)

        def path():
            overlaps()
            _lib.call("mgu_match_masks", dev, B, *sides, scores, thr, th.size, mg, mi, totals)
            _lib.call("mgu_panoptic_totals", dev, B, *sides, C, pq)

        path()
        emit(what="workload", workload=tag, B=B, H=H, W=W, gt_objects=n_gt, pred_objects=n_pred, pairs=int(pairs[0][n_pred]),
             thresholds=int(th.size), status=int(status.item()))
        emit(what="object_overlaps", workload=tag, us=round(timed(overlaps, iters) * 1e3, 1))
        emit(what="device_path", workload=tag, us=round(timed(path, iters) * 1e3, 1))
        if not args.quick:
            totals.zero_(), pq.zero_()
            path()
            h_mg, h_mi, h_tot, h_pq, h_pairs, sec = host_composition(tg, tp, scores, th, C)
            same = (np.array_equal(mg.cpu().numpy(), h_mg) and np.array_equal(mi.cpu().numpy().view(np.uint64), h_mi.view(np.uint64))
                    and np.array_equal(totals.cpu().numpy(), h_tot) and np.array_equal(pq.cpu().numpy().view(np.uint64), h_pq)
                    and int(pairs[0][n_pred]) == h_pairs)
            emit(what="host_composition", workload=tag, us=round(sec * 1e6, 1), same_results=bool(same))


if __name__ == "__main__":
    main()
