"""Deterministic cases, the float64 reference and the error bars for the Lovasz-Softmax kernels (csrc/lovasz.hip), in plain torch /
numpy on the CPU in the style of tests/losses_cases.py, whose Ref, err_of, FLOOR and layout helpers are reused.  Imported by
tests/test_lovasz_host.py (the reference against the set-function definition, closed forms, hand-computed cases: no GPU) and
tests/test_gpu_lovasz.py (the kernels).

The definition is INTEGRATION.md section Q (Berman, Triki, Blaschko, CVPR 2018, written from the paper): per segment -- a class over
the batch, or over one image -- the errors e = 1 - p[c] (label c) / p[c] (else) are ranked in descending order, ties in pixel order;
the loss of the segment is sum_k e_(k) g_k with g the increments of the Jaccard loss along that order, here from integer counts in
closed form.  The ranking is a DECISION: an fp32 and a float64 softmax order a few per cent of the pixels differently, the value is
continuous across a swap and the gradient is not.  So gradients are compared with the device's own ranks pinned (`ranks`): the loss
is then linear in e and autograd gives the gradient of exactly the order the kernel took.

The bars are losses_cases': 4 * cond + 2^-22 with cond the deviation of the SAME code in fp32 (same pinned ranks) from float64, never
above CAP (2e-6 for the value, 5e-6 -- the dice cap -- for gradients and for the device's errors against the float64 softmax)."""
from functools import lru_cache

import numpy as np
import torch

import mgunet_oracle as O
from losses_cases import FLOOR, Ref, autograd_run, err_of, lay_crop, lay_first_of_8, lay_nchw, lay_nhwc  # noqa: F401

CAP = {"value": 2e-6, "grad": 5e-6, "errors": 5e-6}
IGNORE = -100
LAYOUTS = {"nchw": lay_nchw, "nhwc": lay_nhwc, "first_of_8": lay_first_of_8, "crop": lay_crop}
RAW_PITCH, RAW_SCALE, RAW_SCALE_DEV, RAW_PREFILL = 8, 0.5, 1.75, 1e-4


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def jaccard_increments(fg_sorted) -> np.ndarray:
    """g_k for k = 1 .. n along a ranking, fg_sorted[k - 1] = the pixel at rank k is foreground; float64 from integer counts.
    G foreground pixels in all, F_k among ranks 1 .. k, U_k = G + k - F_k:  foreground 1 / U_k;  background (G - F_k) / (U_k (U_k - 1));
    G == 0: 1 at rank 1 and 0 after it."""
    fg = np.asarray(fg_sorted, dtype=bool)
    n, G = len(fg), int(fg.sum())
    g = np.zeros(n, dtype=np.float64)
    if n == 0:
        return g
    if G == 0:
        g[0] = 1.0
        return g
    k = np.arange(1, n + 1, dtype=np.int64)
    F = np.cumsum(fg.astype(np.int64))
    U = (G + k - F).astype(np.float64)
    g[fg] = 1.0 / U[fg]
    bg = ~fg
    g[bg] = (G - F[bg]).astype(np.float64) / (U[bg] * (U[bg] - 1.0))      # U >= G + 1 >= 2 on a background pixel
    return g


def jaccard_loss_of_set(fg, wrong) -> float:
    """The set function the loss extends: 1 - |gt & pred| / |gt | pred| when the pixels of `wrong` are mispredicted (a foreground
    pixel predicted background and the reverse); 0 for an empty union."""
    fg, wrong = np.asarray(fg, dtype=bool), np.asarray(wrong, dtype=bool)
    pred = fg ^ wrong
    union = int((fg | pred).sum())
    return 1.0 - int((fg & pred).sum()) / union if union else 0.0


def lovasz_extension_bruteforce(errors, fg) -> float:
    """sum_k e_(k) * (Delta({(1) .. (k)}) - Delta({(1) .. (k - 1)})) along the descending order of the errors (ties: lower index
    first), every Delta evaluated from the set itself."""
    e, fg = np.asarray(errors, dtype=np.float64), np.asarray(fg, dtype=bool)
    order = np.argsort(-e, kind="stable")
    wrong = np.zeros(len(e), dtype=bool)
    total, before = 0.0, 0.0
    for i in order:
        wrong[i] = True
        now = jaccard_loss_of_set(fg, wrong)
        total += e[i] * (now - before)
        before = now
    return total


def segments(B, per_image):
    """the image groups whose pixels are ranked together"""
    return [(b,) for b in range(B)] if per_image else [tuple(range(B))]


def lovasz_reference(logits, labels, classes="present", per_image=False, ignore_index=IGNORE, ranks=None, dtype=torch.float64):
    """The loss as a torch scalar of `dtype`, differentiable w.r.t. logits (B, C, H, W); labels (B, H, W) int64.  ranks (C, B, H, W)
    integers (-1 on ignored pixels), if given, IS the order inside every segment; otherwise the errors are sorted by the tie rule."""
    B, C = logits.shape[:2]
    p = torch.softmax(logits.to(dtype), dim=1).reshape(B, C, -1)
    y = labels.reshape(B, -1)
    total = p.sum() * 0.0
    groups = segments(B, per_image)
    for grp in groups:
        yb = torch.cat([y[b] for b in grp])
        valid = yb != ignore_index
        terms = []
        for c in range(C):
            fg = (yb == c)[valid]
            if classes == "present" and int(fg.sum()) == 0:
                continue
            pc = torch.cat([p[b, c] for b in grp])[valid]
            e = torch.where(fg, 1.0 - pc, pc)
            if ranks is None:
                order = torch.sort(e.detach(), descending=True, stable=True).indices
            else:
                order = torch.argsort(torch.cat([torch.as_tensor(ranks[c, b]).reshape(-1) for b in grp])[valid].long(), stable=True)
            g = torch.from_numpy(jaccard_increments(fg[order].numpy())).to(dtype)
            terms.append((e[order] * g).sum())
        if terms:
            total = total + sum(terms) / len(terms)
    return total / len(groups)


def softmax_errors(logits, labels, dtype=torch.float64, ignore_index=IGNORE):
    """(C, B, H, W): e of every pixel for every class, 0 on an ignored pixel (what the kernel's hook holds there)"""
    p = torch.softmax(logits.to(dtype), dim=1)
    onehot = labels[:, None] == torch.arange(logits.shape[1])[None, :, None, None]
    e = torch.where(onehot, 1.0 - p, p)
    return torch.where((labels == ignore_index)[:, None], torch.zeros_like(e), e).permute(1, 0, 2, 3)


def differenced_fp32_gradient(errors_sorted, fg_sorted) -> np.ndarray:
    """The published formulation's gradient in fp32: jaccard = 1 - (G - cumsum(fg)) / (G + cumsum(1 - fg)), neighbours differenced."""
    fg = np.asarray(fg_sorted, dtype=np.float32)
    gts = fg.sum(dtype=np.float32)
    inter = gts - np.cumsum(fg, dtype=np.float32)
    union = gts + np.cumsum(np.float32(1.0) - fg, dtype=np.float32)
    jac = np.float32(1.0) - inter / union
    out = jac.copy()
    out[1:] = jac[1:] - jac[:-1]
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def cases(T):
    """tag -> (B, C, H, W, kind, classes, per_image).  T = the keys one workgroup ranks per sort pass (mgu_lovasz_tile): the sizes
    around it are one tile less one, one tile, two tiles, and four tiles (at least three workgroups in the scan and every scatter)."""
    out = {}
    for i, n in enumerate((1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5)):
        out[f"n{n}"] = (1, (2, 3, 5, 8)[i % 4], 1, n, "random", "present", False)
    # B = 3 per image: image 1 lacks the last class, image 2 is ignore_index throughout
    for n, cls in ((64, "present"), (65, "all"), (T + 1, "all"), (3 * T + 5, "present")):
        out[f"image_{cls}_{n}"] = (3, 3, 1, n, "per_image", cls, True)
    out["batch_of_3"] = (3, 5, 1, T + 1, "per_image", "present", False)   # the same labels ranked over the batch: segments of 3 T + 3
    out["ignore"] = (2, 3, 19, 23, "ignore", "present", False)
    out["ignore_image"] = (2, 4, 19, 23, "ignore", "all", True)
    out["saturated"] = (2, 3, 19, 23, "saturated", "present", False)
    out["equal_c2"] = (1, 2, 1, T + 7, "equal", "present", False)
    out["equal_c3"] = (2, 3, 5, 13, "equal", "present", True)
    out["low_digit"] = (1, 2, 1, 700, "low_digit", "present", False)
    out["high_digit"] = (1, 4, 1, T + 9, "high_digit", "present", False)
    out["absent_all"] = (2, 4, 19, 23, "absent", "all", False)
    out["absent_present"] = (2, 4, 19, 23, "absent", "present", False)
    out["one_class_all"] = (1, 3, 7, 11, "one_class", "all", False)
    out["one_class_present"] = (1, 3, 7, 11, "one_class", "present", False)
    out["c1"] = (2, 1, 5, 13, "c1", "present", False)
    out["all_ignored"] = (2, 3, 5, 13, "all_ignored", "present", False)
    out["all_ignored_all"] = (2, 3, 5, 13, "all_ignored", "all", True)
    return out


LAYOUT_TAGS = ("ignore", "ignore_image")
RAW_TAGS = ("ignore", "n65")          # C = 3: the <4> kernel of the final pass, C = 8: the <8> kernel


def low_digit_values(n):
    """n fp32 values in [0.75, 0.75 + 2^-14): the bits of 0.75 with 256 + (37 j mod 512) in the lowest ten"""
    bits = np.uint32(0x3F400000) | (256 + (37 * np.arange(n, dtype=np.uint32)) % 512).astype(np.uint32)
    return bits.view(np.float32)


def inputs(tag, T):
    """(logits fp32 (B, C, H, W), labels int64 (B, H, W), classes, per_image)"""
    B, C, H, W, kind, classes, per_image = cases(T)[tag]
    lg = torch.from_numpy(O.formula_normal(f"lvcase/{tag}/l", (B, C, H, W), seed=C)).clone() * 2.0
    y = torch.from_numpy(O.formula_labels(f"lvcase/{tag}/y", (B, H, W), C, seed=C + 1)).clone()
    flat = torch.arange(B * H * W).reshape(B, H, W)
    if kind == "per_image":
        y[1][y[1] == C - 1] = 0
        y[2] = IGNORE
    elif kind == "ignore":
        y[torch.from_numpy(O.formula_uniform(f"lvcase/{tag}/i", (B, H, W), seed=5)) < 0.2] = IGNORE
    elif kind == "saturated":       # gap 800: exp(-800) is 0 in fp32 AND in float64: every error is exactly 0.0 or 1.0 and the float64
        top = torch.from_numpy(O.formula_labels(f"lvcase/{tag}/a", (B, H, W), C, seed=9))       # gradient identically zero (at a gap of
        lg = torch.full((B, C, H, W), -400.0).scatter_(1, top[:, None], 400.0)                   # 120 it is 1e-52, not zero: nothing to compare)
    elif kind == "equal":
        lg[:] = 0.37
    elif kind == "low_digit":       # every error of both classes is one of low_digit_values up to the rounding of the softmax
        v = torch.from_numpy(low_digit_values(B * H * W).astype(np.float64)).reshape(B, H, W)
        p1 = torch.where(y == 1, 1.0 - v, v)
        lg[:, 0], lg[:, 1] = 0.0, torch.log(p1 / (1.0 - p1)).float()
    elif kind == "high_digit":      # errors 0, 0.25, 0.5, 0.75, 1 exactly: their fp32 bits differ in the top ten key bits only
        kindof, nxt = flat % 4, (y + 1) % C
        sat = torch.full((B, C, H, W), -60.0)
        right = sat.clone().scatter_(1, y[:, None], 60.0)
        wrong = sat.clone().scatter_(1, nxt[:, None], 60.0)
        pair = right.clone().scatter_(1, nxt[:, None], 60.0)
        lg = torch.zeros(B, C, H, W)
        for j, src in ((1, right), (2, wrong), (3, pair)):
            lg = torch.where((kindof == j)[:, None], src, lg)
    elif kind == "absent":
        y[y == C - 1] = 0
    elif kind == "one_class":
        y[:] = 1
    elif kind == "c1":
        y[:] = 0
    elif kind == "all_ignored":
        y[:] = IGNORE
    return lg.float().contiguous(), y.contiguous(), classes, per_image


def reference(tag, T, ranks=None) -> Ref:
    """value and dlogits of the case in float64 (and cond from fp32), with the given ranks pinned"""
    lg, y, classes, per_image = inputs(tag, T)
    return Ref(lambda dt: autograd_run(lambda l: lovasz_reference(l, y, classes, per_image, IGNORE, ranks, dt), [lg], dt, names=["grad"]))


def errors_reference(tag, T) -> Ref:
    lg, y, _, _ = inputs(tag, T)
    return Ref(lambda dt: {"errors": softmax_errors(lg, y, dt)})


def raw_prefill(tag, T):
    B, C, H, W = cases(T)[tag][:4]
    return torch.from_numpy(O.formula_normal(f"lvcase/{tag}/pre", (B * H * W, RAW_PITCH), seed=3)) * RAW_PREFILL


def raw_reference(tag, T, ranks) -> Ref:
    """columns [0, C) after the accumulating call: prefill + grad_scale * (*grad_scale_dev) * dL/dlogits, rows = pixels"""
    B, C, H, W = cases(T)[tag][:4]
    lg, y, classes, per_image = inputs(tag, T)
    pre, k = raw_prefill(tag, T)[:, :C], RAW_SCALE * RAW_SCALE_DEV

    def run(dt):
        r = autograd_run(lambda l: lovasz_reference(l, y, classes, per_image, IGNORE, ranks, dt), [lg], dt, names=["g"])
        return {"value": r["value"], "acc": pre.to(dt) + k * r["g"].permute(0, 2, 3, 1).reshape(B * H * W, C)}
    return Ref(run)


def check_ranks(errors, ranks, labels, per_image, ignore_index=IGNORE):
    """The device's ranks (C, B, H, W) are a valid stable descending sort of the device's errors: per segment a permutation of
    0 .. n - 1 over the pixels that are not ignored, errors non-increasing along it, equal errors in ascending pixel order, -1 on
    ignored pixels.  numpy, exact.  Returns the number of tied neighbours it saw."""
    e, r, y = np.asarray(errors), np.asarray(ranks), np.asarray(labels)
    C, B = e.shape[:2]
    ties = 0
    for grp in segments(B, per_image):
        yb = np.concatenate([y[b].reshape(-1) for b in grp])
        valid = yb != ignore_index
        n = int(valid.sum())
        for c in range(C):
            eb = np.concatenate([e[c, b].reshape(-1) for b in grp])
            rb = np.concatenate([r[c, b].reshape(-1) for b in grp])
            assert (rb[~valid] == -1).all(), ("ignored pixels hold -1", c, grp)
            rv, ev, pix = rb[valid], eb[valid], np.nonzero(valid)[0]
            assert np.array_equal(np.sort(rv), np.arange(n)), ("a permutation of 0 .. n - 1", c, grp)
            order = np.argsort(rv)
            es, ps = ev[order], pix[order]
            assert (es[1:] <= es[:-1]).all(), ("errors non-increasing", c, grp)
            same = es[1:] == es[:-1]
            assert (ps[1:][same] > ps[:-1][same]).all(), ("equal errors in ascending pixel order", c, grp)
            ties += int(same.sum())
    return ties
