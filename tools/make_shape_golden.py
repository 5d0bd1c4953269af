"""Writes tests/golden/shapes.npz: the reference's own EllipticalShapeLoss (model/unet/shape_loss.py) on single shapes, on scenes of
overlapping ellipses with salt noise and on a few edge cases -- the fixture tests/test_shape_host.py and tests/test_gpu_shapes.py pin
mgunet.object_shapes to.

    python tools/make_shape_golden.py --reference <MinGraph-UNet checkout>

Dev-box tool (CPU only; needs numpy, torch and the reference checkout, whose class is loaded from its file at run time); nothing on
the GPU side runs it.  Objects are labelled with the tests' numpy oracle (tests/objects_oracle.py, 8-connectivity, equal values
join), and the reference is called once per object -- loss(None, [[mask]]): with one object per call the value is that object's
term -- and once per image with the whole mask list.

Arrays only.  single_names; single_{k}_bits (256 x 256 mask, np.packbits), single_{k}_ref (float32).  scene_{k}_bits (512 x 512,
packbits), scene_{k}_terms (float32, one per object of >= 10 pixels in label order), scene_{k}_loss (float32).  edge_names;
edge_{k}_map (int8 class map), edge_{k}_terms, edge_{k}_loss as for the scenes; edge_{k}_loss_c1: the reference's loss over the
class-1 objects only (the three-class case).  thin_names; thin_{k}_map (int8): one-pixel diagonal, anti-diagonal and sloped lines and a
two-pixel band, whose covariance is singular or nearly so.  They carry NO reference value and do not enter ref_dev: there the
reference raises on its singular fp32 inverse or returns an epsilon-dominated number, and the tests hold the device to the oracle's
exact rational evaluation instead.  ref_dev: the largest relative deviation, over every stored object, between the
reference's float32 term and the float64 oracle (tests/shapes_oracle.py); the fixture is not written if it exceeds 2e-5, the
tolerance tests/test_gpu_losses_pipeline.py grants this reference class for its float32 accumulation."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import objects_oracle as OO  # noqa: E402
import shapes_oracle as SO  # noqa: E402

REF_DEV_CEILING = 2e-5


def load_reference_loss(root):
    path = os.path.join(root, "model", "unet", "shape_loss.py")
    spec = importlib.util.spec_from_file_location("reference_shape_loss", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.EllipticalShapeLoss()


def ellipse(H, W, cy, cx, ry, rx, theta=0.0):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dy, dx = y - cy, x - cx
    u, v = dx * np.cos(theta) + dy * np.sin(theta), -dx * np.sin(theta) + dy * np.cos(theta)
    return (u / rx) ** 2 + (v / ry) ** 2 <= 1.0


def single_shapes():
    H = W = 256
    out = {"ellipse": ellipse(H, W, 128, 128, 40, 70), "tilted_ellipse": ellipse(H, W, 128, 128, 25, 80, np.deg2rad(30.0))}
    sq = np.zeros((H, W), bool)
    sq[70:160, 90:180] = True
    out["square"] = sq
    out["two_discs"] = ellipse(H, W, 128, 88, 40, 40) | ellipse(H, W, 128, 168, 40, 40)
    el = np.zeros((H, W), bool)
    el[40:200, 60:100] = True
    el[160:200, 60:220] = True
    out["L"] = el
    line = np.zeros((H, W), bool)
    line[77, 100:156] = True
    out["line"] = line
    out["noise"] = np.random.default_rng(3).random((H, W)) < 0.02
    return out


def scene(seed, H=512, W=512, n=40, density=0.002):
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        a, b = rng.uniform(6, 28), rng.uniform(6, 28)
        m |= ellipse(H, W, cy, cx, a, b, rng.uniform(0, np.pi))
    return m | (rng.random((H, W)) < density)


def edge_cases():
    small = np.zeros((32, 32), np.int8)
    small[3:6, 4:7] = 1            # exactly 9 pixels
    small[12:14, 10:15] = 1        # exactly 10 pixels
    run = np.zeros((16, 64), np.int8)
    run[5, 3:51] = 1               # a one-pixel-high run
    full = np.ones((64, 64), np.int8)
    three = np.zeros((96, 128), np.int8)
    three[ellipse(96, 128, 30, 30, 14, 22, 0.4)] = 1
    three[ellipse(96, 128, 62, 84, 18, 11, 1.1)] = 1
    three[ellipse(96, 128, 30, 66, 16, 16)] = 2        # touches the first class-1 ellipse: different values do not join
    three[ellipse(96, 128, 75, 30, 9, 20, 2.5)] = 2
    three[88:91, 100:103] = 1      # 9 pixels, class 1
    three[5:7, 110:113] = 2        # 6 pixels, class 2
    return {"nine_and_ten": small, "row_run": run, "full_image": full, "three_class": three}


def thin_cases():
    """One map of thin objects, none touching another: diagonals of 10, 30 and 100 pixels, anti-diagonals of 10, 30 and 120, a
    slope-2 staircase of 400, a slope-1/3 staircase of 90 and a two-pixel-wide diagonal band of 150 rows."""
    m = np.zeros((448, 448), np.int8)
    for n, r0, c0 in ((10, 5, 5), (30, 5, 30), (100, 5, 80)):
        m[r0 + np.arange(n), c0 + np.arange(n)] = 1
    for n, r0, c0 in ((10, 120, 14), (30, 120, 70), (120, 120, 440)):
        m[r0 + np.arange(n), c0 - np.arange(n)] = 1
    t = np.arange(400)
    m[40 + t, 200 + t // 2] = 1
    t = np.arange(90)
    m[250 + t // 3, 180 + t] = 1
    r = np.arange(260, 410)
    m[r, r - 250] = 1
    m[r, r - 249] = 1
    assert OO.label(m.astype(np.int64), 2).max() == 9
    return {"lines": m}


def reference_terms(ref, labels, keep=None):
    """(float32 terms of the objects of >= 10 pixels in label order, their float64 oracle terms, the reference's loss over the mask
    list -- restricted to the objects with keep[k] true when given)."""
    import torch
    n = int(labels.max())
    masks = [torch.from_numpy(labels == k) for k in range(1, n + 1)]
    orc = SO.shapes_of_labels(labels)
    terms, want = [], []
    for k, m in enumerate(masks):
        if int(m.sum()) >= 10:
            terms.append(float(ref(None, [[m]])))
            want.append(orc[k]["term"])
    sel = [m for k, m in enumerate(masks) if keep is None or keep[k]]
    return np.array(terms, np.float32), np.array(want, np.float64), np.float32(float(ref(None, [sel])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a MinGraph-UNet checkout (contains model/unet/shape_loss.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "shapes.npz"))
    a = ap.parse_args()
    import torch
    ref = load_reference_loss(a.reference)
    arrays, devs = {}, []

    def dev(got, want):
        if len(got):
            devs.append(float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want))))

    singles = single_shapes()
    arrays["single_names"] = np.array(list(singles))
    for k, (name, m) in enumerate(singles.items()):
        ys, xs = np.nonzero(m)
        r = np.float32(float(ref(None, [[torch.from_numpy(m)]])))
        arrays[f"single_{k}_bits"], arrays[f"single_{k}_ref"] = np.packbits(m), r
        dev(np.array([r]), np.array([SO.shape(ys, xs)["term"]]))
        print(f"single {name}: {len(ys)} pixels, reference term {r:.6f}")
    for k, seed in enumerate((7, 8, 9, 10)):
        m = scene(seed)
        labels = OO.label(m.astype(np.int64), 2)
        terms, want, total = reference_terms(ref, labels)
        arrays[f"scene_{k}_bits"], arrays[f"scene_{k}_terms"], arrays[f"scene_{k}_loss"] = np.packbits(m), terms, total
        dev(terms, want)
        area = np.bincount(labels.reshape(-1))[1:]
        print(f"scene seed {seed}: {labels.max()} objects, {len(terms)} of >= 10 pixels, largest {area.max()}, reference loss {total:.4f}")
    edges = edge_cases()
    arrays["edge_names"] = np.array(list(edges))
    for k, (name, m) in enumerate(edges.items()):
        labels = OO.label(m.astype(np.int64), 2)
        terms, want, total = reference_terms(ref, labels)
        cls = OO.stats(labels, m)[0]
        arrays[f"edge_{k}_map"], arrays[f"edge_{k}_terms"], arrays[f"edge_{k}_loss"] = m, terms, total
        arrays[f"edge_{k}_loss_c1"] = reference_terms(ref, labels, keep=(cls == 1))[2]
        dev(terms, want)
        print(f"edge {name}: {labels.max()} objects, {len(terms)} of >= 10 pixels, reference loss {total:.6f}")
    thin = thin_cases()
    arrays["thin_names"] = np.array(list(thin))
    for k, (name, m) in enumerate(thin.items()):
        arrays[f"thin_{k}_map"] = m
        print(f"thin {name}: terms (oracle) {[round(s['term'], 6) for s in SO.shapes_of_labels(OO.label(m.astype(np.int64), 2))]}")
    ref_dev = max(devs)
    print(f"ref_dev = {ref_dev:.3e}")
    if ref_dev > REF_DEV_CEILING:
        raise SystemExit(f"ref_dev {ref_dev:.3e} exceeds {REF_DEV_CEILING}: the oracle disagrees with the reference; nothing written")
    arrays["ref_dev"] = np.array(ref_dev, np.float64)
    np.savez_compressed(a.out, **arrays)
    print(f"wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
