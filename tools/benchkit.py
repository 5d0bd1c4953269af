"""What the bench tools share, each written once: the import path of the package, the tests' oracles and the float64 oracle, the three
ways a tool times a call, the JSON line it prints, and the two synthetic inputs more than one tool uses.  `import benchkit` comes
first in a tool (a script run as `python tools/x.py` has tools/ first on sys.path); the numbers in DESIGN.md and
profiles/*_bench.txt come from these functions.

  timed        ms per call between two HIP events around `iters` calls, all queued behind a parked stream: the GPU's time
  timed_each   median ms of per-call event pairs, every call synchronised: a warm call as a user makes it
  wall         ms per call by the host clock around `iters` calls and one synchronise"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in ("oracle", "tests", "mingraph-unet_amd"):
    if os.path.join(ROOT, _p) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, _p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SPIN_CYCLES = 50_000_000   # the spin kernel only has to outlast the enqueue of `iters` calls; the events do not bracket it


def timed(fn, iters, warmup, park=True):
    """ms per call between two HIP events.  The stream is parked behind a spin kernel first, so that every call is enqueued before
    the first one runs and the events time the GPU, not the host's launch rate.  park=False measures that rate instead: the calls
    run as the host issues them."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if park:
        torch.cuda._sleep(SPIN_CYCLES)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def timed_each(fn, reps, warmup):
    """median ms over `reps` calls, each between its own pair of HIP events and synchronised"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def wall(fn, iters, warmup):
    """ms per call by the host clock: `iters` calls, then one synchronise"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def median_spread(fn, iters, runs, warmup=3):
    """(median, min, max) in microseconds of `runs` timed loops of `iters` calls"""
    us = [timed(fn, iters, warmup) * 1e3 for _ in range(runs)]
    return round(statistics.median(us), 1), round(min(us), 1), round(max(us), 1)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def ellipse_scene(B, H, W, seed):
    """int64 class maps: clusters of overlapping ellipses of class 1."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((B, H, W), np.int64)
    for b in range(B):
        for _ in range(14):
            cy, cx = rng.uniform(40, H - 40), rng.uniform(40, W - 40)
            for _ in range(rng.randint(2, 5)):
                a, e, t = rng.uniform(18, 30), rng.uniform(0.7, 1.0), rng.uniform(0, np.pi)
                oy, ox = cy + rng.uniform(-30, 30), cx + rng.uniform(-30, 30)
                u = (xs - ox) * np.cos(t) + (ys - oy) * np.sin(t)
                v = -(xs - ox) * np.sin(t) + (ys - oy) * np.cos(t)
                out[b][(u / a) ** 2 + (v / (a * e)) ** 2 <= 1.0] = 1
    return out


def logits_of(cmap, C, dev):
    """(B, C, H, W) view of NHWC fp32 logits whose first maximal class is cmap"""
    x = torch.zeros(tuple(cmap.shape) + (C,), dtype=torch.float32)
    x.scatter_(-1, torch.from_numpy(cmap).unsqueeze(-1), 1.0)
    return x.to(dev).permute(0, 3, 1, 2)
