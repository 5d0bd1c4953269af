"""Deterministic cases, float64 references and error bars for the optimizer step whose decisions stay on the device
(csrc/optim.hip: mgu_grad_norm, mgu_optim_step, mgu_grad_accumulate).  Plain torch / numpy on the CPU,
inputs from the oracle's formula tensors: no fixture, no GPU.  Imported by tests/test_optim_cases_host.py (case properties, wrong
variants restated in fp32, schedulers, config mapping) and tests/test_gpu_optim.py (the kernels).

The references are torch itself in float64: torch.nn.utils.clip_grad_norm_ on the scaled gradient, then torch.optim.Adam / AdamW /
SGD (foreach=False), then the EMA recurrence e = d e + (1 - d) p, over chains of three steps from a fresh optimizer.  Measures and
bars are those of tests/step_cases.py (Ref, err_of, opt_cap): a tensor against its largest reference element, p as its UPDATE,
bar = min(4 * cond + 2^-22, opt_cap()) with cond the deviation from float64 of torch's own fp32 run of the same chain.

The sum of squares has a bar of its own: every term is positive, so ANY summation order in double stays within (n - 1) u of the
exact sum relative to it, u = 2^-53, and the squares themselves are exact in double (24-bit operands); the bar is (n + 2) u against
math.fsum of the exact squares."""
import math
from functools import lru_cache

import numpy as np
import torch

import mgunet_oracle as O
from step_cases import ADAM_BETAS, ADAM_EPS, ADAM_LR, OPT_GRID, OPT_SIZES, OPT_STEPS, SGD_LR, Ref, err_of, opt_cap, update_of  # noqa: F401

CLIP_EPS = 1e-6                    # torch.nn.utils.clip_grad_norm_: max_norm / (total_norm + 1e-6)
EMA_DECAY = 0.9


def _normal(name, shape, seed):
    return torch.from_numpy(O.formula_normal(name, shape, seed=seed))


# ---- the gradient norm --------------------------------------------------------------------------------------------------------------
NORM_CONTENTS = ("normal", "one_1e19", "all_1e-30", "zero")
NORM_RUNS = [(c, n) for c in NORM_CONTENTS for n in OPT_SIZES]


def norm_input(content, n):
    """fp32 gradient of n elements.  one_1e19: its square, 1e38, is a factor 3.4 below the largest fp32 value and 44 orders above the others; all_1e-30: every square underflows fp32."""
    if content == "normal":
        return (_normal("ocase/norm/g", (n,), 5) * 1e-2).float()
    if content == "one_1e19":
        g = torch.full((n,), 1e-3)
        g[n // 2] = 1e19
        return g
    if content == "all_1e-30":
        return torch.full((n,), 1e-30)
    assert content == "zero", content
    return torch.zeros(n)


def exact_sumsq(g) -> float:
    """math.fsum of the exact squares (a product of two fp32 values is exact in double)."""
    a = g.double().numpy()
    return math.fsum((a * a).tolist())


@lru_cache(maxsize=None)
def norm_reference(content, n) -> float:
    return exact_sumsq(norm_input(content, n))


def sumsq_bar(n) -> float:
    return (n + 2) * 2.0 ** -53


def sumsq_err(got, ref) -> float:
    if ref == 0.0:
        return 0.0 if got == 0.0 else float("inf")
    return abs(got - ref) / ref


# ---- chains of mgu_optim_step -------------------------------------------------------------------------------------------------------
# tag: (kind, momentum, weight decay, grad_scale, clip, ema decay, ema warmup, magnitude of g, index of a step with a NaN or None)
#   clip "off": max_norm 0;  "half": half the smallest norm of the chain (coef < 1 on every step);  "far": four times the largest
#   (coef == 1 exactly);  "edge": the first step's norm lowered by 5e-4 of itself;  "one": max_norm 1.0 (the huge gradients)
CASES = {
    "adam": ("adam", 0.0, 1e-4, 1.0, "off", 0.0, False, 1e-2, None),
    "adam_clip": ("adam", 0.0, 1e-4, 1.0, "half", EMA_DECAY, False, 1e-2, None),
    "adam_gs8_clip": ("adam", 0.0, 1e-4, 0.125, "half", EMA_DECAY, False, 1e-2, None),
    "adam_skip": ("adam", 0.0, 1e-4, 1.0, "half", EMA_DECAY, False, 1e-2, 1),
    "adamw": ("adamw", 0.0, 1e-2, 1.0, "off", 0.0, False, 1e-2, None),
    "adamw_clip": ("adamw", 0.0, 1e-2, 1.0, "half", EMA_DECAY, False, 1e-2, None),
    "adamw_far": ("adamw", 0.0, 1e-2, 1.0, "far", EMA_DECAY, True, 1e-2, None),
    "adamw_edge": ("adamw", 0.0, 1e-2, 1.0, "edge", 0.0, False, 1e-2, None),
    "sgd_m0": ("sgd", 0.0, 1e-4, 1.0, "off", 0.0, False, 1e-2, None),
    "sgd_m0_clip": ("sgd", 0.0, 1e-4, 1.0, "half", EMA_DECAY, False, 1e-2, None),
    "sgd_m0.9": ("sgd", 0.9, 1e-4, 1.0, "off", 0.0, False, 1e-2, None),
    "sgd_m0.9_clip": ("sgd", 0.9, 1e-4, 1.0, "half", EMA_DECAY, False, 1e-2, None),
    "sgd_huge_clip": ("sgd", 0.9, 0.0, 1.0, "one", 0.0, False, 1e20, None),      # squares of 1e40: a sum kept in fp32 is inf
}
SWEPT = ("adam", "adam_clip", "adamw", "adamw_clip", "sgd_m0", "sgd_m0_clip", "sgd_m0.9", "sgd_m0.9_clip")     # at every n of OPT_SIZES
RUNS = [(t, n) for t in SWEPT for n in OPT_SIZES] + [(t, 100003) for t in CASES if t not in SWEPT]
KIND_CODE = {"adam": 0, "adamw": 1, "sgd": 2}


def lr_of(kind) -> float:
    return SGD_LR if kind == "sgd" else ADAM_LR


def scaled_norm64(g, gs) -> float:
    return abs(gs) * math.sqrt(exact_sumsq(g))


@lru_cache(maxsize=None)
def inputs(tag, n):
    """(p, grads, max_norm): fp32 tensors of n elements; grads has OPT_STEPS finite gradients and, for a case with a bad step, one
    more at that index whose element n // 2 is NaN.  max_norm is a float32 value (the descriptor carries a float)."""
    kind, mom, wd, gs, clip, ema, warm, mag, bad = CASES[tag]
    p = (_normal("scase/adam/p", (n,), 1) * 1e-3).float()
    grads = [(_normal(f"scase/adam/g{i}", (n,), 2) * mag).float() for i in range(OPT_STEPS)]
    norms = [scaled_norm64(g, gs) for g in grads]
    max_norm = {"off": 0.0, "half": 0.5 * min(norms), "far": 4.0 * max(norms), "edge": norms[0] * (1.0 - 5e-4), "one": 1.0}[clip]
    if bad is not None:
        g = grads[0].clone()
        g[n // 2] = float("nan")
        grads.insert(bad, g)
    return p, grads, float(np.float32(max_norm))


def finite(g) -> bool:
    return bool(torch.isfinite(g).all())


def ema_decay_at(decay, warm, t) -> float:
    return min(decay, (1.0 + t) / (10.0 + t)) if warm else decay


def clip_coefs(tag, n):
    """clip_grad_norm_'s factor of every applied step, in float64."""
    gs = CASES[tag][3]
    p, grads, max_norm = inputs(tag, n)
    return [min(1.0, max_norm / (scaled_norm64(g, gs) + CLIP_EPS)) if max_norm > 0 else 1.0 for g in grads if finite(g)]


@lru_cache(maxsize=None)
def reference(tag, n) -> Ref:
    kind, mom, wd, gs, clip, ema, warm, mag, bad = CASES[tag]
    p, grads, max_norm = inputs(tag, n)

    def run(dt):
        w = torch.nn.Parameter(p.to(dt).clone())
        if kind == "sgd":
            opt = torch.optim.SGD([w], lr=SGD_LR, momentum=mom, weight_decay=wd, foreach=False)
        else:
            cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
            opt = cls([w], lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=wd, foreach=False)
        e, t = p.to(dt).clone(), 0
        for g in grads:
            if not finite(g):                                 # skip_nonfinite: the step does not happen
                continue
            t += 1
            w.grad = g.to(dt) * gs
            if max_norm > 0:
                torch.nn.utils.clip_grad_norm_([w], max_norm)
            opt.step()
            d = ema_decay_at(ema, warm, t)
            e = d * e + (1.0 - d) * w.detach()
        out = {"p": update_of(w.detach(), p)}
        if kind == "sgd":
            if mom:
                out["buf"] = opt.state[w]["momentum_buffer"]
        else:
            out["m"], out["v"] = opt.state[w]["exp_avg"], opt.state[w]["exp_avg_sq"]
        if ema:
            out["ema"] = e
        return out
    return Ref(run)


VARIANTS = ("kernel", "l2_for_decoupled", "clip_unscaled_norm", "clip_after_decay", "attempted_step_count", "sumsq_fp32")


def formula32(tag, n, variant="kernel"):
    """The arithmetic of optim_control_kernel and optim_update_kernel in numpy (the control in float64 cast once, the update in
    fp32), or one of the wrong variants the bars have to catch.  For the host test only.  Same keys as reference()."""
    assert variant in VARIANTS, variant
    f = np.float32
    kind, mom, wd, gs, clip, ema, warm, mag, bad = CASES[tag]
    p0, grads, max_norm = inputs(tag, n)
    if variant == "l2_for_decoupled" and kind == "adamw":
        kind = "adam"
    lr = f(lr_of(kind))
    b1, b2, omb1, omb2 = f(ADAM_BETAS[0]), f(ADAM_BETAS[1]), f(1.0 - ADAM_BETAS[0]), f(1.0 - ADAM_BETAS[1])
    eps, wdf, momf = f(ADAM_EPS), f(wd), f(mom)
    keep = f(1.0 - float(lr) * float(wdf))
    p = p0.numpy().copy()
    m, v, e = np.zeros(n, f), np.zeros(n, f), p.copy()
    step = attempts = 0
    for g in grads:
        g = g.numpy()
        attempts += 1
        if not np.isfinite(g).all():
            continue
        step += 1
        if variant == "sumsq_fp32":
            with np.errstate(over="ignore"):
                sumsq = float(np.sum(g * g, dtype=f))
        else:
            sumsq = float(np.sum(g.astype(np.float64) ** 2))
        norm = (1.0 if variant == "clip_unscaled_norm" else abs(gs)) * math.sqrt(sumsq)
        coef = min(1.0, max_norm / (norm + CLIP_EPS)) if max_norm > 0 else 1.0
        t = attempts if variant == "attempted_step_count" else step
        bc1, bc2s = f(1.0 - ADAM_BETAS[0] ** t), f(math.sqrt(1.0 - ADAM_BETAS[1] ** t))
        d = f(ema_decay_at(float(f(ema)), warm, t))
        if variant == "clip_after_decay" and kind != "adamw":
            gi = (g * f(gs) + wdf * p) * f(coef)
        else:
            gi = g * f(gs * coef)
            if kind == "adamw":
                p = p * keep
            else:
                gi = gi + wdf * p
        if kind == "sgd":
            if mom:
                gi = gi if step == 1 else momf * m + gi
                m = gi
            p = p - lr * gi
        else:
            m = b1 * m + omb1 * gi
            v = b2 * v + omb2 * gi * gi
            p = p - (lr / bc1) * m / (np.sqrt(v) / bc2s + eps)
        e = d * e + (f(1) - d) * p
        assert p.dtype == f and m.dtype == f and v.dtype == f and e.dtype == f
    out = {"p": update_of(p, p0)}
    if kind == "sgd":
        if mom:
            out["buf"] = m
    else:
        out["m"], out["v"] = m, v
    if ema:
        out["ema"] = e
    return out


def outside_bar(tag, n, variant) -> bool:
    """The variant misses the bar of at least one of the case's quantities."""
    ref, cap, got = reference(tag, n), opt_cap(), formula32(tag, n, variant)
    return any(err_of(k, got[k], ref.r64[k]) > ref.bar(k, cap) for k in ref.r64)


# ---- schedulers ---------------------------------------------------------------------------------------------------------------------
class LrHolder:
    """What a scheduler of mgunet.engine needs of a Trainer."""

    def __init__(self, lr):
        self.lr = lr

    def set_lr(self, lr):
        self.lr = lr


# (mode, threshold_mode, metrics): plateaus longer than the patience, improvements below the threshold, a cooldown, the floor min_lr
# and a last reduction smaller than eps
PLATEAU_KW = dict(factor=0.5, patience=2, threshold=1e-2, cooldown=1, min_lr=1.2e-4, eps=1e-5)
PLATEAU_SCRIPTS = [
    ("min", "rel", [1.0, 0.9, 0.895, 0.894, 0.893, 0.8, 0.81, 0.82, 0.83, 0.84, 0.85, 0.86, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5,
                    0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),
    ("min", "abs", [1.0, 0.995, 0.993, 0.98, 0.98, 0.98, 0.98, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]),
    ("max", "rel", [0.1, 0.2, 0.2005, 0.201, 0.2015, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3]),
    ("max", "abs", [0.1, 0.105, 0.109, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.2]),
]
