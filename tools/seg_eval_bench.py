"""Segmentation evaluation at the flagship shape (UNet(3, 2, 32, 4), 8 x 3 x 512 x 512, C = 2), one process, one GPU:

  forward ms | forward + SegmentationEvaluator.update ms | eval kernel us (HIP events, per loss kind, with / without the
  prediction map) | the reference's host path: argmax on the device, D2H of predictions and masks, confusion on the host.

Prints one JSON line per measurement.  Run under `rocprofv3 --kernel-trace --stats -- python tools/seg_eval_bench.py` for the
per-kernel times (profiles/seg_eval_kernel_stats.csv)."""
import time

from benchkit import emit, timed  # first: benchkit sets the import path
import numpy as np
import torch

import mgunet
import mgunet_oracle as O
from mgunet.metrics import confusion_matrix_host

def main():
    dev = torch.device("cuda:0")
    B, H, W, C = 8, 512, 512, 2
    cfg = (3, C, 32, 4)
    model = mgunet.UNet(*cfg)
    model.load_state_dict(O.make_unet_params(*cfg, seed=1))
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, 3, H, W), generator=g).to(dev)
    y = torch.randint(0, C, (B, H, W), generator=g).to(dev)
    ev = mgunet.SegmentationEvaluator(C, dev)
    with torch.no_grad():
        fwd = timed(lambda: model(x), 20, 5, park=False)
        fwd_upd = timed(lambda: ev.update(model(x)[0], y), 20, 5, park=False)
        logits = model(x)[0]
    emit(what="forward", B=B, H=H, W=W, C=C, ms=round(fwd, 4))
    emit(what="forward+update", ms=round(fwd_upd, 4), overhead_ms=round(fwd_upd - fwd, 4))
    nbytes = logits.numel() * 4 + y.numel() * 8
    for loss in (None, "ce", "ce+dice"):
        e = mgunet.SegmentationEvaluator(C, dev, loss=loss)
        for pred in (False, True):
            ms = timed(lambda: e.update(logits, y, return_pred=pred), 200, 20)
            extra = B * H * W * 8 if pred else 0
            emit(what="eval_kernels", loss=loss, pred_map=pred, us=round(ms * 1e3, 2), bytes=nbytes + extra,
                 tb_per_s=round((nbytes + extra) / (ms * 1e-3) / 1e12, 3))
        e.compute()
    # the reference's path (segmentation_performance.py:141-151): argmax on the device, both maps to the host, confusion there
    def host_path():
        pred = mgunet.argmax_classes(logits)
        t0 = time.perf_counter()
        pv, yv = pred.view(-1).cpu(), y.view(-1).cpu()
        t1 = time.perf_counter()
        confusion_matrix_host(yv.numpy(), pv.numpy(), C)
        t2 = time.perf_counter()
        sk = None
        try:
            from sklearn.metrics import confusion_matrix
            confusion_matrix(yv.numpy(), pv.numpy(), labels=list(range(C)))
            sk = (time.perf_counter() - t2) * 1e3
        except ImportError:
            pass
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, sk
    host_path()
    runs = [host_path() for _ in range(3)]
    emit(what="host_path", d2h_ms=round(float(np.median([r[0] for r in runs])), 3),
         numpy_confusion_ms=round(float(np.median([r[1] for r in runs])), 3),
         sklearn_confusion_ms=None if runs[0][2] is None else round(float(np.median([r[2] for r in runs])), 3))
    ev.compute()


if __name__ == "__main__":
    main()
