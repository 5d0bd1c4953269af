"""Frame registration and object tracks (csrc/video.hip) on a short clip, one process, one GPU: 8 x 512 x 512 x 3 uint8 frames of a
synthetic scene -- discs of two classes on a textured ground, seen by a camera that drifts by a known shift per frame, with fresh
noise on every frame -- registered at factor 2, radius 24, then linked and numbered.

Rows, each the device time of the call as the median of --runs timed loops of 20 calls with their spread (HIP events around calls
queued behind a parked stream: the GPU's time, not the host's launch rate):
  (a) copy          a device copy of the frame bytes: what reading the clip once costs at the least
  (b) registration  mgu_frame_shifts alone, with its split into the plane, SAD and pick kernels from the context's profiling records
  (c) tracks        mgu_track_align + mgu_object_overlaps + mgu_match_masks + mgu_track_ids on the clip's labelled objects and shifts
  (d) both          (b) then (c)
  (e) torch         the same registration composed from torch on the device: the luma and block means, then a loop over the shifts of
                    (a - b.roll(shift)).abs().sum() on the window, the same tie rule; the shifts must be identical
  (f) numpy         the oracle of the tests on the host (wall clock, one call); the shifts must be identical
One JSON line per measurement.  --quick: fewer iterations."""
import argparse
import time

from benchkit import emit, median_spread  # first: benchkit sets the import path
import numpy as np
import torch

import mgunet
import video_oracle as VO
from mgunet import _lib
from mgunet import video as V

R, F = 24, 2
DRIFT = [(-6, -30), (4, -22), (-2, -37), (7, -26), (-5, -31), (3, -18), (-8, -41)]       # the true [dy, dx] of the seven pairs


def clip(T, H, W):
    """frames uint8 (T, H, W, 3), class maps int64 (T, H, W), true shifts (T-1, 2)"""
    rng = np.random.RandomState(0)
    cam = np.cumsum([(0, 0)] + [(-dy, -dx) for dy, dx in DRIFT[:T - 1]], axis=0)
    cam -= cam.min(0)
    WH, WW = H + int(cam[:, 0].max()), W + int(cam[:, 1].max())
    ground = rng.randint(40, 120, (WH // 8 + 1, WW // 8 + 1, 3)).repeat(8, 0).repeat(8, 1)[:WH, :WW].astype(np.float32)
    ground += rng.normal(0, 12, ground.shape)
    cls = np.zeros((WH, WW), np.int64)
    yy, xx = np.mgrid[:WH, :WW]
    for _ in range(60):
        cy, cx, r, c = rng.uniform(20, WH - 20), rng.uniform(20, WW - 20), rng.uniform(9, 18), rng.randint(1, 3)
        m = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        cls[m] = c
        ground[m] = (225, 60, 50) if c == 1 else (235, 190, 40)
    frames = np.stack([ground[y:y + H, x:x + W] for y, x in cam]) + rng.normal(0, 6, (T, H, W, 3))
    return np.clip(frames, 0, 255).astype(np.uint8), np.stack([cls[y:y + H, x:x + W] for y, x in cam]), np.asarray(DRIFT[:T - 1], np.int32)


def tie_rank(r, dev):
    """(2r+1)^2 ranks of the shifts in (sy^2 + sx^2, sy, sx) order"""
    keys = sorted((sy * sy + sx * sx, sy, sx) for sy in range(-r, r + 1) for sx in range(-r, r + 1))
    rank = {(sy, sx): i for i, (_, sy, sx) in enumerate(keys)}
    return torch.tensor([rank[(sy, sx)] for sy in range(-r, r + 1) for sx in range(-r, r + 1)], device=dev)


def torch_registration(frames, dev):
    """the composition a user would write on the device"""
    T, H, W, _ = frames.shape
    w = torch.tensor([77, 150, 29], device=dev, dtype=torch.int32)
    rank_c, rank_f = tie_rank(R, dev), tie_rank(F, dev)

    def level(a, b, M, r, rank):
        """a, b (P, h, w) int32 -> (P,) flat index of the chosen shift in [-r, r]^2"""
        h, wd = a.shape[1:]
        cost = torch.stack([(a[:, M:h - M, M:wd - M] - b.roll((-sy, -sx), (1, 2))[:, M:h - M, M:wd - M]).abs().sum((1, 2))
                            for sy in range(-r, r + 1) for sx in range(-r, r + 1)], 1)
        return (cost * rank.numel() + rank).argmin(1)

    def run():
        y = ((frames.to(torch.int32) * w).sum(-1) + 128) >> 8
        c = (y[:, :H // F * F, :W // F * F].reshape(T, H // F, F, W // F, F).sum((2, 4)) + F * F // 2) // (F * F)
        i = level(c[:-1], c[1:], R, R, rank_c)
        centre = torch.stack([i // (2 * R + 1) - R, i % (2 * R + 1) - R], 1) * F
        moved = torch.stack([y[t + 1].roll((-cy, -cx), (0, 1)) for t, (cy, cx) in enumerate(centre.tolist())])      # reads the centre back
        j = level(y[:-1], moved, F * R + F, F, rank_f)
        return centre + torch.stack([j // (2 * F + 1) - F, j % (2 * F + 1) - F], 1)
    return run


def stage_split(ctx, run, reps):
    L = _lib.lib()
    out = {}
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        for _ in range(reps):
            run()
            torch.cuda.synchronize()
            once = {}
            for k in _lib.read_kernel_stats(ctx):
                once[k["name"]] = once.get(k["name"], 0.0) + k["ms"] * 1e3
            for k, v in once.items():
                out.setdefault(k, []).append(v)
    finally:
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return {k: round(float(np.median(v)), 1) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = _lib.context(dev)
    T, H, W = 8, 512, 512
    iters, runs = (3, 2) if args.quick else (20, args.runs)
    emit(what="setup", sad_tile=int(_lib.lib().mgu_frame_sad_tile()), iters=iters, loops=runs, T=T, H=H, W=W, radius=R, factor=F)
    frames_np, cls_np, truth = clip(T, H, W)
    frames = torch.from_numpy(frames_np).to(dev)
    table = mgunet.connected_components(torch.from_numpy(cls_np).to(dev))
    N = table.class_id.numel()
    shifts = torch.empty((T - 1, 2), device=dev, dtype=torch.int32)
    cost = torch.empty((T - 1, 2), device=dev, dtype=torch.int64)

    def registration():
        _lib.call("mgu_frame_shifts", dev, frames, T, H, W, 3, 0, R, F, shifts, cost, None)

    registration()
    got = shifts.cpu().numpy()
    emit(what="shifts", kernel=got.tolist(), truth=truth.tolist(), equal_truth=bool(np.array_equal(got, truth)), cost=cost.cpu().tolist())

    bufs = V._link_buffers(dev, N, (T - 1) * H * W)
    thr = torch.tensor([0.3], dtype=torch.float64).to(dev)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    ids = torch.empty(N, device=dev, dtype=torch.int64)
    next_id = torch.zeros(1, device=dev, dtype=torch.int64)
    tlen, tcls = torch.zeros(N, device=dev, dtype=torch.int32), torch.empty(N, device=dev, dtype=torch.int64)

    def tracks():
        next_id.zero_()
        tlen.zero_()
        link = V._link(table.labels, table.offsets, table.class_id, N, shifts, T, H, W, thr, None, bufs, status)
        V._ids(table.offsets, T, N, link, table.class_id, None, next_id, ids, tlen, tcls, status)

    def both():
        registration()
        tracks()

    tracks()
    emit(what="tracks", objects=N, tracks=int(next_id), counted=int((tlen >= 2).sum()), status=int(status))
    other = frames.clone()
    base, blo, bhi = median_spread(lambda: other.copy_(frames), iters, runs)
    emit(what="device", row="a copy", bytes=frames.numel(), us={"median": base, "min": blo, "max": bhi})
    ours = {}
    for name, fn in (("b registration", registration), ("c tracks", tracks), ("d both", both)):
        med, lo, hi = median_spread(fn, iters, runs)
        ours[name] = med
        emit(what="device", row=name, us={"median": med, "min": lo, "max": hi}, over_copy=round(med / base, 1), stages_us=stage_split(ctx, fn, 5))
    composed = torch_registration(frames, dev)
    tshift = composed().cpu().numpy()
    tmed, tlo, thi = median_spread(composed, 1 if args.quick else 3, min(runs, 3), warmup=1)
    emit(what="torch_composition", row="e torch", identical_shifts=bool(np.array_equal(tshift, got)), us={"median": tmed, "min": tlo, "max": thi},
         torch_over_kernel=round(tmed / ours["b registration"], 1))
    t0 = time.perf_counter()
    oshift = VO.frame_shifts(frames_np, R, F)[0]
    emit(what="numpy_oracle", row="f numpy", identical_shifts=bool(np.array_equal(oshift, got)), wall_ms=round((time.perf_counter() - t0) * 1e3, 1))


if __name__ == "__main__":
    main()
