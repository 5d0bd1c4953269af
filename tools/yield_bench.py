"""Object counting at 8 x 512^2 and 32 x 1024^2, C = 2, one process, one GPU.  The maps hold random discs (a few hundred objects
per image, some touching) and the logits are one-hot on them:

  labelling us (int64 class map; fused logits argmax) | stats us | YieldEvaluator.update us (GT + prediction labelling, stats
  and matching) | the host path: D2H of the argmax predictions + labelling on the CPU (scipy.ndimage.label, when installed).

Prints one JSON line per measurement.  Run under `rocprofv3 --kernel-trace --stats -- python tools/yield_bench.py` for the
per-kernel times (profiles/objects_kernel_stats.csv)."""
import time

from benchkit import emit, timed  # first: benchkit sets the import path
import numpy as np
import torch

import mgunet
from mgunet import objects as mobj


def discs(B, H, W, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((B, H, W), np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    n = H * W // 1200
    for b in range(B):
        for cy, cx, r in zip(rng.integers(0, H, n), rng.integers(0, W, n), rng.integers(4, 14, n)):
            y0, y1, x0, x1 = max(0, cy - r), min(H, cy + r + 1), max(0, cx - r), min(W, cx + r + 1)
            m[b, y0:y1, x0:x1] |= ((yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2 <= r * r)
    return m


def main():
    dev = torch.device("cuda:0")
    C = 2
    for B, H, W in ((8, 512, 512), (32, 1024, 1024)):
        cmap = torch.from_numpy(discs(B, H, W, B)).to(dev)
        logits = torch.nn.functional.one_hot(cmap, C).float().contiguous().permute(0, 3, 1, 2)
        nhwc = logits.permute(0, 2, 3, 1)
        labels = torch.empty((B, H, W), device=dev, dtype=torch.int32)
        counts = torch.empty(B, device=dev, dtype=torch.int64)
        offsets = torch.empty(B + 1, device=dev, dtype=torch.int64)
        lab_map = timed(lambda: mobj._label(cmap, 0, B, H, W, 0, 2, 0, 0, 0, labels, counts, offsets), 50, 5)
        lab_fused = timed(lambda: mobj._label(nhwc, 1, B, H, W, C, 2, 0, 0, 0, labels, counts, offsets), 50, 5)
        N = int(offsets[B])
        cls = torch.empty(N, device=dev, dtype=torch.int64)
        area = torch.empty(N, device=dev, dtype=torch.int64)
        bbox = torch.empty((N, 4), device=dev, dtype=torch.int32)
        sums = torch.empty((N, 2), device=dev, dtype=torch.int64)
        st = timed(lambda: mobj._stats(labels, nhwc, 1, B, H, W, C, offsets, N, cls, bbox, area, sums), 50, 5)
        ev = mgunet.YieldEvaluator(C, dev)
        upd = timed(lambda: ev.update(logits, cmap), 20, warmup=2)
        emit(what="objects", B=B, H=H, W=W, C=C, objects_per_image=round(N / B, 1), label_classmap_us=round(lab_map * 1e3, 1),
             label_fused_logits_us=round(lab_fused * 1e3, 1), stats_us=round(st * 1e3, 1), evaluator_update_us=round(upd * 1e3, 1),
             classmap_read_gb=round(cmap.numel() * 8 / 1e9, 4))
        ev.compute()

        def host_path():
            pred = mgunet.argmax_classes(logits)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pv = pred.cpu().numpy()
            t1 = time.perf_counter()
            lab = None
            try:
                from scipy import ndimage
                st8 = ndimage.generate_binary_structure(2, 2)
                for b in range(B):
                    ndimage.label(pv[b], structure=st8)
                lab = (time.perf_counter() - t1) * 1e3
            except ImportError:
                pass
            return (t1 - t0) * 1e3, lab
        host_path()
        runs = [host_path() for _ in range(3)]
        emit(what="host_path", B=B, H=H, W=W, d2h_ms=round(float(np.median([r[0] for r in runs])), 3),
             scipy_label_ms=None if runs[0][1] is None else round(float(np.median([r[1] for r in runs])), 3))


if __name__ == "__main__":
    main()
