"""Deterministic cases, the float64 reference and the error bars for the pixel cross-entropy kernels (csrc/pixel_ce.hip), in plain
torch / numpy on the CPU in the style of tests/losses_cases.py, whose Ref, err_of, FLOOR and layout helpers are reused.  Imported by
tests/test_pixel_ce_host.py (the reference against F.cross_entropy, hand-computed cases, the selection oracle: no GPU) and
tests/test_gpu_pixel_ce.py (the kernels).

The definition is INTEGRATION.md section S.  Per counted pixel l = (1 - eps) w_y (-lp_y) + (eps / C) sum_c w_c (-lp_c), or with the
focal term l = w_y (1 - p_y)^gamma (-lp_y); per group (the batch, or one image) the K = min(n, max(min_kept, ceil(f n))) pixels of
largest l are kept, equal l in pixel order; L = sum_kept l / sum_kept w_y.  Which pixels are kept is a DECISION: an fp32 and a float64
softmax order pixels of nearly equal loss differently, and with weights the value is not continuous across a swap.  So value and
gradient are compared with the device's own kept map pinned (`kept`), and the selection itself is checked exactly against the
oracle run on the device's own fp32 losses.

The bars are losses_cases': 4 * cond + 2^-22 with cond the deviation of the SAME code in fp32 (same pinned kept map) from float64,
never above CAP (2e-6 for the value, 5e-6 -- the dice cap -- for gradients and for the per-pixel loss plane)."""
import math
from functools import lru_cache

import numpy as np
import torch

import mgunet_oracle as O
from losses_cases import FLOOR, Ref, autograd_run, err_of, lay_crop, lay_first_of_8, lay_nchw, lay_nhwc  # noqa: F401

CAP = {"value": 2e-6, "grad": 5e-6, "plane": 5e-6}
IGNORE = -100
LAYOUTS = {"nchw": lay_nchw, "nhwc": lay_nhwc, "first_of_8": lay_first_of_8, "crop": lay_crop}
RAW_PITCH, RAW_SCALE, RAW_SCALE_DEV, RAW_PREFILL = 8, 0.5, 1.75, 1e-4
VARIANTS = ("mean_count", "unweighted_smoothing", "ties_high", "floor_k", "rank_py", "focal_p")   # wrong readings of the definition


def options(weight=None, eps=0.0, gamma=0.0, keep=1.0, min_kept=0, per_image=False):
    return {"weight": None if weight is None else tuple(float(w) for w in weight), "eps": float(eps), "gamma": float(gamma),
            "keep": float(keep), "min_kept": int(min_kept), "per_image": bool(per_image)}


def api_kwargs(opt, device=None):
    """the keyword arguments of mgunet.pixel_cross_entropy for an options dict"""
    w = None if opt["weight"] is None else torch.tensor(opt["weight"], dtype=torch.float32, device=device)
    return {"weight": w, "label_smoothing": opt["eps"], "focal_gamma": opt["gamma"], "keep_fraction": opt["keep"],
            "min_kept": opt["min_kept"], "per_image": opt["per_image"]}


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def kept_count(n, keep, min_kept, variant=None) -> int:
    """K = min(n, max(min_kept, ceil(keep * n))), product and ceil in IEEE double"""
    byf = math.floor(float(keep) * float(n)) if variant == "floor_k" else math.ceil(float(keep) * float(n))
    return min(int(n), max(int(min_kept), int(byf)))


def groups(B, per_image):
    return [(b,) for b in range(B)] if per_image else [tuple(range(B))]


def select(loss, counted, keep, min_kept, per_image, variant=None) -> np.ndarray:
    """The kept map (B, H, W) int32 of the tie rule: 1 kept, 0 dropped, -1 not counted.  loss (B, H, W) of any float type is ranked as
    it is (the device's fp32 plane, or a float64 reference); keep == 1 keeps every counted pixel."""
    loss, counted = np.asarray(loss), np.asarray(counted, dtype=bool)
    B = loss.shape[0]
    out = np.where(counted, 0, -1).astype(np.int32)
    flat = out.reshape(B, -1)
    for grp in groups(B, per_image):
        vals = np.concatenate([loss[b].reshape(-1) for b in grp])
        cnt = np.concatenate([counted[b].reshape(-1) for b in grp])
        idx = np.nonzero(cnt)[0]
        if keep == 1.0:
            take = idx
        else:
            K = kept_count(len(idx), keep, min_kept, variant)
            if variant == "ties_high":
                order = len(idx) - 1 - np.argsort(-vals[idx][::-1], kind="stable")
            else:
                order = np.argsort(-vals[idx], kind="stable")
            take = idx[order[:K]]
        hw = flat.shape[1]
        flat[np.asarray(grp)[take // hw], take % hw] = 1
    return out


def select_bruteforce(loss, counted, keep, min_kept, per_image) -> np.ndarray:
    """the same map from a sort of (-loss, pixel index) pairs in plain Python"""
    loss, counted = np.asarray(loss), np.asarray(counted, dtype=bool)
    B = loss.shape[0]
    out = np.where(counted, 0, -1).astype(np.int32)
    for grp in groups(B, per_image):
        pairs = []
        for b in grp:
            lb, cb = loss[b].reshape(-1), counted[b].reshape(-1)
            pairs += [(-float(lb[i]), b, i) for i in range(len(lb)) if cb[i]]
        pairs.sort()
        K = len(pairs) if keep == 1.0 else kept_count(len(pairs), keep, min_kept)
        for _, b, i in pairs[:K]:
            out[b].reshape(-1)[i] = 1
    return out


def pixel_losses(logits, labels, opt, ignore_index=IGNORE, dtype=torch.float64, variant=None):
    """(l (B, H, W) with 0 on the pixels that are not counted, w_y (B, H, W), p_y (B, H, W)): torch of `dtype`, differentiable"""
    B, C = logits.shape[:2]
    x = logits.to(dtype)
    nlp = -torch.log_softmax(x, dim=1)
    w = torch.ones(C, dtype=dtype) if opt["weight"] is None else torch.tensor(opt["weight"], dtype=dtype)
    counted = labels != ignore_index
    ys = torch.where(counted, labels, torch.zeros_like(labels))
    nlp_y = nlp.gather(1, ys[:, None])[:, 0]
    wy = w[ys]
    p = torch.softmax(x, dim=1)
    onehot = ys[:, None] == torch.arange(C)[None, :, None, None]
    py = (p * onehot).sum(1)
    if opt["gamma"] == 0.0:
        sw = torch.ones(C, dtype=dtype) if variant == "unweighted_smoothing" else w
        l = (1.0 - opt["eps"]) * wy * nlp_y + (opt["eps"] / C) * (sw[None, :, None, None] * nlp).sum(1)
    else:
        miss = (p * ~onehot).sum(1)                          # 1 - p_y without the cancellation
        l = wy * (py if variant == "focal_p" else miss) ** opt["gamma"] * nlp_y
    zero = torch.zeros_like(l)
    return torch.where(counted, l, zero), torch.where(counted, wy, zero), py


def pixel_ce_reference(logits, labels, opt, kept=None, ignore_index=IGNORE, dtype=torch.float64, variant=None):
    """The loss as a torch scalar of `dtype`, differentiable w.r.t. logits (B, C, H, W); labels (B, H, W) int64.  kept (B, H, W)
    integers, if given, IS the kept set (entries == 1); otherwise the reference selects by its own losses."""
    l, wy, py = pixel_losses(logits, labels, opt, ignore_index, dtype, variant)
    if kept is None:
        rank_by = (1.0 - py.detach()) if variant == "rank_py" else l.detach()
        kept = select(rank_by.numpy(), (labels != ignore_index).numpy(), opt["keep"], opt["min_kept"], opt["per_image"], variant)
    m = torch.as_tensor(np.asarray(kept) == 1)
    zero = torch.zeros_like(l)
    num = torch.where(m, l, zero).sum()
    den = float(m.sum()) if variant == "mean_count" else torch.where(m, wy, zero).sum()
    return num / den


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
W4 = (0.5, 2.0, 0.0, 1.25)        # class 2 carries no weight


def weights_for(C):
    """C weights >= 0 around 1, the third one 0 where there is a third class"""
    return tuple((0.5, 2.0, 0.0, 1.25, 0.75, 3.0, 1.5, 0.25)[c] for c in range(C))


@lru_cache(maxsize=None)
def cases(T):
    """tag -> (B, C, H, W, kind, options).  T = the keys one workgroup counts per pass (mgu_pixel_ce_tile): the group sizes around it
    are one tile less one, one tile, one more, and two tiles and a piece (three workgroups in every pass and in the tie scan)."""
    out = {}
    mine = [options(keep=0.25), options(weight=weights_for(3), eps=0.1, keep=1.0 / 3.0), options(gamma=2.0, keep=0.25),
            options(weight=weights_for(8), keep=0.5, min_kept=10)]
    for i, n in enumerate((1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 17)):
        out[f"n{n}"] = (1, (2, 3, 5, 8)[i % 4], 1, n, "random", mine[i % 4])
    # B = 3: image 2 is ignore_index throughout; ranked per image and over the batch
    out["image_of_3"] = (3, 3, 1, T + 1, "per_image", options(keep=0.25, per_image=True))
    out["image_of_3_weights"] = (3, 3, 1, T + 1, "per_image", options(weight=weights_for(3), eps=0.1, keep=0.3, min_kept=5, per_image=True))
    out["batch_of_3"] = (3, 3, 1, T + 1, "per_image", options(keep=0.25))
    for C in range(1, 9):
        out[f"c{C}"] = (2, C, 19, 23, "ignore", options(weight=weights_for(C), eps=0.1, keep=0.3))
    # the key's edges
    out["equal"] = (1, 2, 1, T + 7, "equal", options(keep=0.25))
    out["equal_image"] = (2, 3, 5, 13, "equal", options(keep=0.4, per_image=True))
    out["straddle"] = (1, 2, 1, 2 * T, "straddle", options(keep=1e-9, min_kept=230))
    out["saturated_top"] = (2, 3, 19, 23, "saturated", options(keep=0.5))      # K inside the tie of the wrong pixels (l = 120)
    out["saturated_zero"] = (2, 3, 19, 23, "saturated", options(keep=0.8))     # K inside the tie of the right ones (l = +0)
    out["low_digit"] = (1, 2, 1, 700, "low_digit", options(keep=0.25))
    out["high_digit"] = (1, 3, 1, T + 9, "high_digit", options(keep=0.3))
    out["k1"] = (1, 4, 1, T + 5, "random", options(keep=1e-9))
    # every option alone and with mining on top, then all of them
    alone = {"plain": {}, "weights": {"weight": W4}, "smooth": {"eps": 0.1}, "focal2": {"gamma": 2.0}, "focal1_sure": {"gamma": 1.0},
             "weights_smooth": {"weight": W4, "eps": 0.1}, "weights_focal": {"weight": W4, "gamma": 2.0}}
    for name, kw in alone.items():
        kind = "sure" if name == "focal1_sure" else "ignore"
        out[f"opt_{name}"] = (2, 4, 19, 23, kind, options(**kw))
        out[f"opt_{name}_mined"] = (2, 4, 19, 23, kind, options(keep=0.3, **kw))
    out["opt_all_image"] = (2, 4, 19, 23, "ignore", options(weight=W4, eps=0.1, keep=0.3, min_kept=50, per_image=True))
    out["opt_min_kept"] = (2, 4, 19, 23, "ignore", options(keep=0.01, min_kept=200))
    return out


LAYOUT_TAGS = ("opt_weights_smooth_mined", "opt_all_image")
RAW_TAGS = ("opt_weights_smooth_mined", "c3", "c6", "opt_focal2")     # C = 4, 3: the <4> kernels, C = 6: the <8> kernels; no select
STRADDLE_HARD, STRADDLE_TIE = 50, (100, 200)    # hard pixels; the tie's pixels before / from the tile boundary; min_kept - hard = 180


def inputs(tag, T):
    """(logits fp32 (B, C, H, W), labels int64 (B, H, W), options)"""
    B, C, H, W, kind, opt = cases(T)[tag]
    lg = torch.from_numpy(O.formula_normal(f"pcecase/{tag}/l", (B, C, H, W), seed=C)).clone() * 2.0
    y = torch.from_numpy(O.formula_labels(f"pcecase/{tag}/y", (B, H, W), C, seed=C + 1)).clone()
    flat = torch.arange(B * H * W).reshape(B, H, W)
    if kind == "per_image":
        y[2] = IGNORE
    elif kind in ("ignore", "sure"):
        y[torch.from_numpy(O.formula_uniform(f"pcecase/{tag}/i", (B, H, W), seed=5)) < 0.2] = IGNORE
        if kind == "sure":          # p_y exactly 1 in fp32 AND in float64 (exp(-1600) is 0 in both) on every seventh pixel
            sure = ((flat % 7) == 3) & (y != IGNORE)
            sat = torch.full((B, C, H, W), -800.0).scatter_(1, y.clamp_min(0)[:, None], 800.0)
            lg = torch.where(sure[:, None], sat, lg)
    elif kind == "equal":
        lg[:] = 0.37
    elif kind == "straddle":        # l = ln 2 on [T - 100, T + 200), large on 50 pixels of the first tile, small elsewhere
        right = torch.full((B, C, H, W), -2.5).scatter_(1, y[:, None], 2.5)
        tie = (flat >= T - STRADDLE_TIE[0]) & (flat < T + STRADDLE_TIE[1])
        hard = ((flat % 61) == 7) & (flat < 61 * STRADDLE_HARD) & ~tie
        lg = torch.where(hard[:, None], -right, right)
        lg = torch.where(tie[:, None], torch.zeros_like(lg), lg)
    elif kind == "saturated":       # gap 120: a right pixel's loss is exactly +0 in fp32 (and 8e-53 in float64), a wrong one's 120
        top = torch.from_numpy(O.formula_labels(f"pcecase/{tag}/a", (B, H, W), C, seed=9))
        lg = torch.full((B, C, H, W), -60.0).scatter_(1, top[:, None], 60.0)
    elif kind == "low_digit":       # label 0 against logits (0, 8 + j 2^-20): l = 8 + j ulp + log1p(exp(-8)), neighbours one ulp apart
        x = np.float32(8.0) + ((37 * np.arange(B * H * W)) % 128).astype(np.float32) * np.float32(2.0 ** -20)
        lg[:, 0], lg[:, 1] = 0.0, torch.from_numpy(x).reshape(B, H, W)
        y[:] = 0
    elif kind == "high_digit":      # the label's logit a below the top one, a in {0, 128, 256, 512, 1024}: l = a exactly in fp32
        a = torch.tensor([0.0, 128.0, 256.0, 512.0, 1024.0])[flat % 5]
        nxt = (y + 1) % C
        lg = torch.full((B, C, H, W), -2000.0).scatter_(1, nxt[:, None], 0.0)
        lg = lg.scatter_(1, y[:, None], -a[:, None])
        lg = torch.where((a == 0)[:, None], torch.full((B, C, H, W), -2000.0).scatter_(1, y[:, None], 0.0), lg)
    return lg.float().contiguous(), y.contiguous(), opt


def reference(tag, T, kept=None, variant=None) -> Ref:
    """value and dlogits of the case in float64 (and cond from fp32), with the given kept map pinned"""
    lg, y, opt = inputs(tag, T)
    return Ref(lambda dt: autograd_run(lambda l: pixel_ce_reference(l, y, opt, kept, IGNORE, dt, variant), [lg], dt, names=["grad"]))


def plane_reference(tag, T) -> Ref:
    lg, y, opt = inputs(tag, T)
    return Ref(lambda dt: {"plane": pixel_losses(lg, y, opt, IGNORE, dt)[0]})


def raw_prefill(tag, T):
    B, C, H, W = cases(T)[tag][:4]
    return torch.from_numpy(O.formula_normal(f"pcecase/{tag}/pre", (B * H * W, RAW_PITCH), seed=3)) * RAW_PREFILL


def raw_reference(tag, T, kept, accumulate=True) -> Ref:
    """columns [0, C) after the call: [prefill +] grad_scale * (*grad_scale_dev) * dL/dlogits, rows = pixels"""
    B, C, H, W = cases(T)[tag][:4]
    lg, y, opt = inputs(tag, T)
    pre, k = raw_prefill(tag, T)[:, :C], RAW_SCALE * RAW_SCALE_DEV

    def run(dt):
        r = autograd_run(lambda l: pixel_ce_reference(l, y, opt, kept, IGNORE, dt), [lg], dt, names=["g"])
        g = k * r["g"].permute(0, 2, 3, 1).reshape(B * H * W, C)
        return {"value": r["value"], "acc": pre.to(dt) + g if accumulate else g}
    return Ref(run)
