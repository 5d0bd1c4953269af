"""Writes tests/golden/seg_metrics.npz: inputs and outputs of the reference's own segmentation_metrics
(experiments/metrics.py:6-69, sklearn confusion matrix) on the cases tests/test_seg_metrics_host.py pins mgunet.metrics to.

    python tools/make_seg_metrics_golden.py --reference <MinGraph-UNet checkout>

Dev-box tool (needs torch, numpy and sklearn, and the reference checkout); nothing on the GPU side runs it.  The fixture holds
arrays only: case k has k_true, k_pred (int64), k_C, k_smooth, and the reference's k_cm, k_iou, k_precision, k_recall, k_f1
(per class, float64) and k_means (mean iou, precision, recall, f1)."""
import argparse
import importlib.util
import os
import warnings

import numpy as np


def load_reference_metrics(root):
    path = os.path.join(root, "experiments", "metrics.py")
    spec = importlib.util.spec_from_file_location("reference_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases():
    rng = np.random.default_rng(2024)
    out = [(np.array([0, 1, 0, 1, 1, 0]), np.array([0, 1, 1, 1, 0, 0]), 2, 1e-6)]   # metrics.py:258-262
    for C in (1, 2, 3, 5, 16):                                                          # random, every smoothing
        n = int(rng.integers(500, 5000))
        t, p = rng.integers(0, C, n), rng.integers(0, C, n)
        for smooth in (1e-6, 0.0, 1.0):
            out.append((t, p, C, smooth))
    t = rng.choice([0, 2], 3000)                                                         # classes 1, 3, 4 absent from both
    p = rng.choice([0, 2], 3000)
    for smooth in (1e-6, 0.0, 1.0):
        out.append((t, p, 5, smooth))
    t = rng.choice([0, 1, 2], 4000)                                                      # -100 and out-of-range labels
    t[rng.random(4000) < 0.1] = -100
    t[rng.random(4000) < 0.05] = 3
    t[rng.random(4000) < 0.02] = 17
    p = rng.integers(0, 3, 4000)
    for smooth in (1e-6, 0.0):
        out.append((t, p, 3, smooth))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a MinGraph-UNet checkout (contains experiments/metrics.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "seg_metrics.npz"))
    a = ap.parse_args()
    import torch
    ref = load_reference_metrics(a.reference)
    arrays = {}
    cs = cases()
    for k, (t, p, C, smooth) in enumerate(cs):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = ref.segmentation_metrics(torch.from_numpy(t.astype(np.int64)), torch.from_numpy(p.astype(np.int64)), C, smooth=smooth)
        arrays[f"{k}_true"], arrays[f"{k}_pred"] = t.astype(np.int64), p.astype(np.int64)
        arrays[f"{k}_C"], arrays[f"{k}_smooth"] = np.array(C, np.int64), np.array(smooth, np.float64)
        arrays[f"{k}_cm"] = np.asarray(r["confusion_matrix"], np.int64)
        for key in ("iou", "precision", "recall", "f1"):
            arrays[f"{k}_{key}"] = np.array(r[f"{key}_per_class"], np.float64)
        arrays[f"{k}_means"] = np.array([r["mean_iou"], r["mean_precision"], r["mean_recall"], r["mean_f1"]], np.float64)
    arrays["ncases"] = np.array(len(cs), np.int64)
    np.savez_compressed(a.out, **arrays)
    print(f"wrote {a.out}: {len(cs)} cases")


if __name__ == "__main__":
    main()
