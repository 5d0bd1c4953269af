"""Writes tests/golden/objects.npz: the reference's own yield_estimation_metrics (experiments/metrics.py:160-253) on the reference's
__main__ inputs and on random cases, and scipy.ndimage.label on a set of masks in both connectivities -- the fixtures
tests/test_yield_metrics_host.py and tests/test_gpu_objects.py pin mgunet.objects to.

    python tools/make_yield_golden.py --reference <MinGraph-UNet checkout>

Dev-box tool (needs numpy, scipy, torch and sklearn -- the reference's metrics module imports them -- and the reference checkout);
nothing on the GPU side runs it.  The reference's function reads a global `smooth` it never defines (NameError); this tool puts
smooth = 1e-6 (segmentation_metrics' default) into the loaded module's globals before calling it.  Its __main__ calls the function
with misspelled keywords (gt_c=, pred_c=); the case here passes the same values positionally.

scipy.ndimage.label joins every nonzero pixel regardless of value; skimage.measure.label joins only equal values.  A multi-class
map is therefore labelled one value at a time with scipy and the objects renumbered in raster order of their first pixel, which is
skimage's (and scipy's) numbering.

Arrays only.  Metrics case k: k_gt, k_pred (counts), k_lists (1 if object lists are passed), k_thresh, k_gto (rows: image, xmin,
ymin, xmax, ymax, class, occluded: -1 absent / 0 / 1), k_pro (rows: image, xmin, ymin, xmax, ymax, class), k_prc (confidence per
prediction row, NaN = absent), k_nimg, and the reference's k_out: count accuracy, yield error, matching rate, occlusion robustness,
total GT, total predicted (float64).  Label case j: lab_j_mask (int64) and lab_j_c1, lab_j_c2 (int32 labels, connectivity 1 / 2)."""
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
    mod.smooth = 1e-6   # read as a global by yield_estimation_metrics and never defined there
    return mod


def random_objects(rng, nimg, pred):
    rows, conf = [], []
    for i in range(nimg):
        for _ in range(int(rng.integers(0, 7))):
            x0, y0 = (int(v) for v in rng.integers(0, 12, 2))
            w, h = (int(v) for v in rng.integers(1, 7, 2))
            c = int(rng.integers(1, 3))
            if pred:
                rows.append([i, x0, y0, x0 + w, y0 + h, c])
                conf.append(float(rng.choice([0.9, 0.5, 0.5])) if rng.random() < 0.3 else np.nan)
            else:
                rows.append([i, x0, y0, x0 + w, y0 + h, c, int(rng.choice([-1, -1, 0, 1]))])
    return np.array(rows, np.int64).reshape(-1, 6 if pred else 7), np.array(conf, np.float64)


def metric_cases():
    rng = np.random.default_rng(7)
    cases = [([10, 12, 8, 15], [9, 13, 7, 14], None)]                                    # metrics.py __main__
    gto = np.array([[0, 10, 10, 50, 50, 0, 0], [0, 60, 60, 100, 100, 0, 1], [1, 20, 20, 70, 70, 0, 0]], np.int64)
    pro = np.array([[0, 12, 12, 48, 48, 0], [0, 50, 50, 90, 90, 0], [1, 25, 25, 75, 75, 0], [1, 100, 100, 120, 120, 0]], np.int64)
    cases.append(([2, 1], [2, 2], (gto, pro, np.array([0.9, 0.8, 0.95, 0.7]), 0.5)))
    cases.append(([0, 0, 0], [0, 0, 0], None))                                            # every GT count zero
    cases.append(([0, 0], [1, 0], None))
    cases.append(([], [], None))
    # exactly 1/2: [0,0,4,2] against [0,0,4,4] (inter 8, union 16); a tie: two GT boxes at the same IoU
    gto = np.array([[0, 0, 0, 4, 4, 1, -1], [0, 0, 0, 4, 4, 1, -1], [0, 10, 10, 12, 12, 2, -1]], np.int64)
    pro = np.array([[0, 0, 0, 4, 2, 1], [0, 0, 2, 4, 4, 1], [0, 10, 10, 12, 12, 1]], np.int64)
    for thresh in (0.5, 0.5000001):
        cases.append(([3], [3], (gto, pro, np.full(3, np.nan), thresh)))
    cases.append(([0, 0], [0, 0], (np.zeros((0, 7), np.int64), np.zeros((0, 6), np.int64), np.zeros(0), 0.5)))   # no objects
    for _ in range(24):
        nimg = int(rng.integers(1, 6))
        gto, _ = random_objects(rng, nimg, False)
        pro, prc = random_objects(rng, nimg, True)
        gt = np.bincount(gto[:, 0], minlength=nimg).tolist() if len(gto) else [0] * nimg
        pr = np.bincount(pro[:, 0], minlength=nimg).tolist() if len(pro) else [0] * nimg
        cases.append((gt, pr, (gto, pro, prc, float(rng.choice([0.5, 0.3, 0.75])))))
    return cases


def to_lists(nimg, gto, pro, prc):
    g = [[] for _ in range(nimg)]
    p = [[] for _ in range(nimg)]
    for r in gto:
        d = {"bbox": [int(v) for v in r[1:5]], "class_id": int(r[5])}
        if r[6] >= 0:
            d["occluded"] = bool(r[6])
        g[r[0]].append(d)
    for r, c in zip(pro, prc):
        d = {"bbox": [int(v) for v in r[1:5]], "class_id": int(r[5])}
        if not np.isnan(c):
            d["confidence"] = float(c)
        p[r[0]].append(d)
    return g, p


def spiral(n):
    m = np.zeros((n, n), np.int64)
    y0, x0, y1, x1 = 0, 0, n - 1, n - 1
    while y0 <= y1 and x0 <= x1:
        m[y0, x0:x1 + 1] = 1
        m[y0:y1 + 1, x1] = 1
        if y1 - y0 >= 2:
            m[y1, x0:x1 + 1] = 1
        if x1 - x0 >= 2:
            m[y0 + 2:y1 + 1, x0] = 1
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    return m


def label_masks():
    rng = np.random.default_rng(11)
    out = [(rng.random((64, 64)) < d).astype(np.int64) for d in (0.3, 0.5, 0.6)]
    snake = np.zeros((100, 130), np.int64)                                       # a 1-pixel serpentine over many 32 x 32 tiles
    for r in range(0, 100, 2):
        snake[r, 1:129] = 1
        snake[r + 1, 128 if (r // 2) % 2 == 0 else 1] = 1 if r + 1 < 100 else 0
    out.append(snake)
    out.append(spiral(97))
    out.append(((np.arange(40)[:, None] + np.arange(40)[None, :]) % 2).astype(np.int64))   # checkerboard
    d = np.zeros((96, 96), np.int64)                                              # diagonals across tile corners
    d[np.arange(96), np.arange(96)] = 1
    d[np.arange(96), 95 - np.arange(96)] = 2
    d[np.arange(0, 96, 3), (np.arange(0, 96, 3) * 7) % 96] = 3
    out.append(d)
    blocks = rng.integers(0, 4, (13, 18)).repeat(4, 0).repeat(4, 1)[:50, :70]   # multi-class blocky map
    blocks[rng.random(blocks.shape) < 0.1] = rng.integers(0, 4)
    out.append(blocks.astype(np.int64))
    out.append(rng.integers(0, 3, (45, 61)).astype(np.int64))                    # multi-class noise
    ring = np.zeros((33, 33), np.int64)
    ring[4:29, 4:29] = 1
    ring[8:25, 8:25] = 0
    ring[14:19, 14:19] = 5
    out.append(ring)
    out += [np.ones((1, 1), np.int64), (rng.random((1, 77)) < 0.5).astype(np.int64), (rng.random((77, 1)) < 0.5).astype(np.int64)]
    return out


def scipy_label(m, connectivity):
    from scipy import ndimage
    st = ndimage.generate_binary_structure(2, connectivity)
    tmp = np.zeros(m.shape, np.int64)
    nxt = 0
    for v in np.unique(m):
        if v == 0:
            continue
        lab, n = ndimage.label(m == v, structure=st)
        tmp[lab > 0] = lab[lab > 0] + nxt
        nxt += n
    flat = tmp.reshape(-1)
    ids, first = np.unique(flat, return_index=True)
    keep = ids > 0
    order = np.argsort(first[keep], kind="stable")
    remap = np.zeros(nxt + 1, np.int64)
    remap[ids[keep][order]] = np.arange(1, keep.sum() + 1)
    return remap[flat].reshape(m.shape).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a MinGraph-UNet checkout (contains experiments/metrics.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "objects.npz"))
    a = ap.parse_args()
    ref = load_reference_metrics(a.reference)
    arrays = {}
    cs = metric_cases()
    for k, (gt, pr, lists) in enumerate(cs):
        arrays[f"{k}_gt"], arrays[f"{k}_pred"] = np.array(gt, np.int64), np.array(pr, np.int64)
        arrays[f"{k}_lists"] = np.array(int(lists is not None), np.int64)
        arrays[f"{k}_nimg"] = np.array(len(gt), np.int64)
        if lists is None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                r = ref.yield_estimation_metrics(gt, pr)
            arrays[f"{k}_thresh"] = np.array(0.5)
            arrays[f"{k}_gto"], arrays[f"{k}_pro"], arrays[f"{k}_prc"] = np.zeros((0, 7), np.int64), np.zeros((0, 6), np.int64), np.zeros(0)
        else:
            gto, pro, prc, thresh = lists
            g, p = to_lists(len(gt), gto, pro, prc)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                r = ref.yield_estimation_metrics(gt, pr, g, p, matching_iou_thresh=thresh)
            arrays[f"{k}_thresh"] = np.array(thresh)
            arrays[f"{k}_gto"], arrays[f"{k}_pro"], arrays[f"{k}_prc"] = gto, pro, prc
        arrays[f"{k}_out"] = np.array([r["count_accuracy_perc"], r["yield_estimation_error_perc"], r["object_matching_rate_perc"],
                                       r["occlusion_robustness_perc"], r["total_gt_count_sum"], r["total_pred_count_sum"]], np.float64)
    arrays["ncases"] = np.array(len(cs), np.int64)
    ms = label_masks()
    for j, m in enumerate(ms):
        arrays[f"lab_{j}_mask"] = m
        arrays[f"lab_{j}_c1"], arrays[f"lab_{j}_c2"] = scipy_label(m, 1), scipy_label(m, 2)
    arrays["nlab"] = np.array(len(ms), np.int64)
    np.savez_compressed(a.out, **arrays)
    print(f"wrote {a.out}: {len(cs)} metric cases, {len(ms)} label cases")


if __name__ == "__main__":
    main()
