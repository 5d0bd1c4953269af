"""Masks in and out at the flagship batch, one process, one GPU: B = 8 images of 512 x 512.

  scene         the overlapping ellipses of benchkit.ellipse_scene split into objects (the scene of the other object benches)
  checkerboard  every other pixel, 8-connected: one object per image with H*W/2 runs and 2*H*W corners in thousands of loops
  full          one full-frame object per image: one run, one loop of 4 corners

For each: the device time of every entry point -- mgu_mask_runs, mgu_runs_to_labels, mgu_object_outlines, mgu_polygons_to_labels --
and of the encode + outline pair, on label maps and tables already on the device (HIP events around calls queued behind a parked
stream: the GPU's time), as the median, min and max of 5 loops of 20 calls; beside them a device copy of the label map.  Then the host
composition each replaces, wall clock, once: the label map copied to the host, the runs by np.diff on the column-major flattening
(one pass per image over object-index changes), the outlines by the numpy oracle (tests/maskio_oracle.py; scene and full only: the
dictionary walk needs minutes on the checkerboard), the polygon fill by matplotlib's point-in-path test per loop combined even-odd (whole
pixel corners, where it agrees with the centre rule), and the copy back.  The results are compared first.  One JSON line per
measurement.  --quick: fewer iterations, no host run."""
import argparse
import time

import benchkit
import numpy as np
import torch
from benchkit import ellipse_scene, emit, median_spread

import mgunet
from mgunet import _lib


def host_runs(labels, offsets):
    """np.diff-based RLE of every object: (run_ptr, start, length), wall-clock seconds included in the caller's timing"""
    B, H, W = labels.shape
    ptr, starts, lengths = [np.zeros(1, np.int64)], [], []
    for b in range(B):
        n = int(offsets[b + 1] - offsets[b])
        flat = labels[b].flatten(order="F")
        flat = np.where((flat >= 1) & (flat <= n), flat, 0)
        edge = np.nonzero(np.diff(np.concatenate(([0], flat, [0]))))[0]            # every change of label
        s, e = edge[:-1], edge[1:]
        keep = flat[s] > 0
        s, e, k = s[keep], e[keep], flat[s[keep]]
        order = np.argsort(k, kind="stable")
        starts.append(s[order]), lengths.append(e[order] - s[order])
        ptr.append(ptr[-1][-1] + np.cumsum(np.bincount(k, minlength=n + 1)[1:]))
    return np.concatenate(ptr), np.concatenate(starts).astype(np.int32), np.concatenate(lengths).astype(np.int32)


def host_fill(polys, B, H, W):
    """matplotlib's point-in-path test at the pixel centres of every loop's box, the loops of an object combined even-odd; corners are
    whole pixels and centres are not, so no centre lies on an edge and the test agrees with the device's rule"""
    from matplotlib.path import Path
    out = np.zeros((B, H, W), np.int32)
    for b, per in enumerate(polys):
        for k, loops in enumerate(per, 1):
            cover = np.zeros((H, W), bool)
            for loop in loops:
                x0, y0, x1, y1 = int(loop[:, 0].min()), int(loop[:, 1].min()), int(loop[:, 0].max()), int(loop[:, 1].max())
                ys, xs = np.mgrid[y0:y1, x0:x1]
                inside = Path(loop.astype(np.float64)).contains_points(np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], 1))
                cover[y0:y1, x0:x1] ^= inside.reshape(y1 - y0, x1 - x0)
            out[b][cover] = np.maximum(out[b][cover], k)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = 8, 512, 512
    iters, runs = (3, 2) if args.quick else (20, 5)
    yy, xx = np.mgrid[0:H, 0:W]
    maps = (("scene", ellipse_scene(B, H, W, 1), True), ("checkerboard", np.broadcast_to(((yy + xx) % 2 == 0).astype(np.int64), (B, H, W)).copy(), False),
            ("full", np.ones((B, H, W), np.int64), False))
    for tag, cmap, split in maps:
        make = mgunet.split_objects if split else mgunet.connected_components
        table = make(torch.from_numpy(cmap).to(dev))
        N, n = table.class_id.numel(), B * H * W
        mk = lambda k, dt: torch.zeros(k, device=dev, dtype=dt)  # noqa: E731
        st = mk(1, torch.int32)
        rp, rs, rl = mk(N + 1, torch.int64), mk(n, torch.int32), mk(n, torch.int32)
        lp, vp, vs, a2 = mk(N + 1, torch.int64), mk(n + 1, torch.int64), mk(8 * n, torch.int32), mk(n, torch.int64)
        back, copy = mk(n, torch.int32), mk(n, torch.int32)
        lab, off = table.labels, table.offsets
        calls = {
            "mask_runs": lambda: _lib.call("mgu_mask_runs", dev, lab, off, N, B, H, W, n, rp, rs, rl, st),
            "runs_to_labels": lambda: _lib.call("mgu_runs_to_labels", dev, rp, rs, rl, n, off, N, B, H, W, back, st),
            "object_outlines": lambda: _lib.call("mgu_object_outlines", dev, lab, off, N, B, H, W, 2, n, 4 * n, lp, vp, vs, a2, st),
            "polygons_to_labels": lambda: _lib.call("mgu_polygons_to_labels", dev, lp, vp, vs, n, 4 * n, off, N, B, H, W, 0, 2 * n, back, st),
        }
        calls["encode_and_outline"] = lambda: (calls["mask_runs"](), calls["object_outlines"]())
        calls["label_map_copy"] = lambda: copy.copy_(lab.view(-1))
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        emit(what="workload", workload=tag, B=B, H=H, W=W, objects=N, runs=int(rp[N]), loops=int(lp[N]), vertices=int(vp[int(lp[N])]),
             status=int(st.item()), fill_round_trip=bool(torch.equal(back.view(B, H, W), lab)))
        for what, fn in calls.items():
            med, lo, hi = median_spread(fn, iters, runs)
            emit(what=what, workload=tag, us=med, min_us=lo, max_us=hi)
        if args.quick:
            continue
        import maskio_oracle as MO
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_lab, h_off = lab.cpu().numpy(), off.cpu().numpy()
        t_in = time.perf_counter() - t0
        t0 = time.perf_counter()
        h_ptr, h_start, h_len = host_runs(h_lab, h_off)
        for a in (h_ptr, h_start, h_len):
            torch.from_numpy(a).to(dev)
        torch.cuda.synchronize()
        R = int(rp[N])
        same = np.array_equal(rp.cpu().numpy(), h_ptr) and np.array_equal(rs[:R].cpu().numpy(), h_start) and np.array_equal(rl[:R].cpu().numpy(), h_len)
        emit(what="host_runs", workload=tag, us=round((t_in + time.perf_counter() - t0) * 1e6, 1), same_results=bool(same))
        if tag != "checkerboard":
            t0 = time.perf_counter()
            o = MO.outlines(h_lab, h_off, 2)
            for a in o:
                torch.from_numpy(a).to(dev)
            torch.cuda.synchronize()
            sec = t_in + time.perf_counter() - t0
            L, V = len(o[3]), len(o[2])
            same = (np.array_equal(lp.cpu().numpy(), o[0]) and np.array_equal(vp[:L + 1].cpu().numpy(), o[1])
                    and np.array_equal(vs.view(-1, 2)[:V].cpu().numpy(), o[2]) and np.array_equal(a2[:L].cpu().numpy(), o[3]))
            emit(what="host_outlines", workload=tag, us=round(sec * 1e6, 1), same_results=bool(same))
            polys = mgunet.OutlineTable(lp, vp, vs.view(-1, 2), a2, st, off, (B, H, W), 2).to_polygons()
            t0 = time.perf_counter()
            h_fill = host_fill(polys, B, H, W)
            torch.from_numpy(h_fill).to(dev)
            torch.cuda.synchronize()
            emit(what="host_fill", workload=tag, us=round((time.perf_counter() - t0) * 1e6, 1), same_results=bool(np.array_equal(h_fill, h_lab)))


if __name__ == "__main__":
    main()
