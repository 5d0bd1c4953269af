"""Deterministic cases, float64 references and error bars for the kernels every training run reports and applies: the segmentation
loss (csrc/train_kernels.hip: ce_fwd_bwd_kernel behind mgu_cross_entropy), the validation loss of mgu_segmentation_eval
(csrc/seg_eval.hip) and the optimizer steps (mgu_adam_step, mgu_sgd_step), on the logits and weights of a TRAINED network: margins
of 6 to 20 between the label class and the rest, losses of 1e-2 to 1e-9, weights of 1e-3.  Plain torch / numpy on the CPU, inputs
from the oracle's formula tensors: no fixture, no GPU.  Imported by tests/test_step_cases_host.py (case properties, the old
formulas restated, no GPU) and tests/test_gpu_step_f64.py (the kernels).

The bars are those of tests/losses_cases.py (Ref, err_of) with one change: a loss is measured relative to ITSELF,

    loss       |v - v64| / |v64|                (0 / inf where v64 == 0 and v is / is not; NaN equals NaN)
    tensor     max|g - g64| / max|g64|          (gradients, Adam's m and v, SGD's buffer)
    p          the tensor measure of the UPDATE p - p_start, i.e. max|p - p64| / max|p64 - p_start|
    bar        min(4 * cond + 2^-22, CAP)

with cond the deviation from float64 of torch's own fp32 run of the same reference (F.cross_entropy, torch.optim.Adam / SGD with
foreach=False).  The max(1, |v64|) denominator of losses_cases.py would hide every error this file is about.  CAP: a loss 1e-6,
the relative bar tests/test_gpu_backward_kernels.py and tests/test_gpu_seg_eval.py hold at random logits; a gradient 2e-5, the
TOL of test_gpu_backward_kernels.py; an optimizer result the 5e-7 absolute of test_gpu_train.py::test_adam_kernel_exact divided by
the largest update of that test's case (opt_cap()).  Where the float64 gradient is identically zero the kernel's has to be
exactly zero."""
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

import losses_cases as LC
import mgunet_oracle as O

FLOOR = LC.FLOOR
LOSS_CAP = 1e-6                    # test_cross_entropy_ignore_index_and_label_range, test_loss_matches_float64_and_is_reproducible
GRAD_CAP = 2e-5                    # TOL of tests/test_gpu_backward_kernels.py
ADAM_EXISTING_BAR = 5e-7           # test_adam_kernel_exact: absolute on p
IGNORE = -100


def err_of(name: str, got, ref64) -> float:
    """losses_cases.err_of, except that `loss` is a scalar measured relative to itself."""
    if name != "loss":
        return LC.err_of(name, got, ref64)
    g, r = float(LC._np64(got)), float(LC._np64(ref64))
    if np.isnan(r) or np.isnan(g):
        return 0.0 if np.isnan(r) and np.isnan(g) else float("inf")
    if r == 0.0:
        return 0.0 if g == 0.0 else float("inf")
    return abs(g - r) / abs(r)


class Ref(LC.Ref):
    measure = staticmethod(err_of)


def _normal(name, shape, seed):
    return torch.from_numpy(O.formula_normal(name, shape, seed=seed))


# ---- cross-entropy ------------------------------------------------------------------------------------------------------------------
CE_GRID_FWD = 2048 * 256           # launch_ce: ce_fwd_bwd_kernel runs at most 2048 workgroups of 256
CE_GRID_COUNT = 1024 * 256         # launch_ce: ce_count_kernel at most 1024
CE_M = (1, 63, 257, 5000, CE_GRID_COUNT + 1, CE_GRID_FWD + 1)
CE_CLASSES = (1, 2, 3, 4, 5, 8, 12)
CE_MARGINS = {"right6": 6.0, "right12": 12.0, "right16": 16.0, "right20": 20.0}
CE_REGIMES = ("random", "right6", "right12", "right16", "right20", "wrong12", "late", "shift100", "shift1000", "huge", "dead",
              "equal")
CE_IGNORES = ("none", "seventh", "all_but_one", "all")
CE_SCALES = (1.0, 0.125)           # the caller's grad_scale, as a factor on the gradient of the mean loss
CE_GRID = 2.0 ** -16               # right12 / shift100 logits are multiples of it: adding 100 is exact in fp32
DEAD_LOGIT = -1e30


def _raise_label_class(lg, y, by):
    lg[torch.arange(lg.shape[0]), y] += by
    return lg


def ce_inputs(regime, C, M, ignore="none"):
    """(logits (M, C) fp32, labels (M,) int64).  The key of the formula tensors leaves the ignore pattern out: the patterns of one
    (regime, C, M) share their logits."""
    key = f"scase/ce/{regime if regime != 'shift100' else 'right12'}/{C}/{M}"
    y = torch.from_numpy(O.formula_labels(key + "/y", (M,), C, seed=C + 1)).clone()
    n = _normal(key + "/l", (M, C), C)
    if regime == "random":
        lg = 3.0 * n
    elif regime in CE_MARGINS or regime == "shift100":
        if regime in ("right12", "shift100"):
            n = torch.round(n / CE_GRID) * CE_GRID
        lg = _raise_label_class(n, y, CE_MARGINS.get(regime, 12.0))
        if regime == "shift100":
            lg = lg + 100.0
    elif regime == "wrong12":
        lg = _raise_label_class(n, y, -12.0)
    elif regime == "late":                       # every tenth pixel still as at the start of training
        lg = _raise_label_class(n.clone(), y, 12.0)
        lg[::10] = 3.0 * n[::10]
    elif regime == "shift1000":
        lg = _raise_label_class(n, y, 3.0) + 1000.0
    elif regime == "huge":
        lg = 3e4 * n
    elif regime == "dead":                       # the last class is dead and never a label
        y = torch.from_numpy(O.formula_labels(key + "/y", (M,), max(C - 1, 1), seed=C + 1)).clone()
        lg = 3.0 * n
        lg[:, C - 1] = DEAD_LOGIT
    elif regime == "equal":
        lg = n[:, :1].expand(M, C).clone()
    else:
        raise KeyError(regime)
    if ignore == "seventh":
        y[::7] = IGNORE
    elif ignore == "all_but_one":
        keep = M // 2
        y[:keep] = IGNORE
        y[keep + 1:] = IGNORE
    elif ignore == "all":
        y[:] = IGNORE
    else:
        assert ignore == "none", ignore
    return lg.float().contiguous(), y


def _ce_cases():
    cases = []
    for regime in CE_REGIMES:                    # every regime at C = 2 and 3
        for C in (2, 3):
            cases.append((regime, C, 5000, "seventh"))
    for C in CE_CLASSES:                         # every C at random and right12
        if C not in (2, 3):
            cases += [("random", C, 257, "none"), ("right12", C, 257, "none")]
    for M in CE_M:                               # every M, both grid caps passed
        if M != 5000:
            cases += [("random", 3, M, "none"), ("right12", 3, M, "none")]
    for ig in CE_IGNORES:                        # every ignore pattern
        if ig != "none":
            cases += [("random", 3, 257, ig), ("right12", 3, 257, ig)]
    cases.append(("shift100", 3, 257, "none"))   # the partner of ("right12", 3, 257, "none") in the shift property
    return cases


CE_CASES = _ce_cases()
CE_SHIFT_PAIRS = [(("right12", C, M, ig), ("shift100", C, M, ig)) for (r, C, M, ig) in CE_CASES if r == "shift100"]


@lru_cache(maxsize=None)
def ce_reference(regime, C, M, ignore) -> Ref:
    """loss = F.cross_entropy (mean over the counted pixels, ignore_index -100) and dlogits = d loss / d logits.  With every pixel
    ignored the loss is 0 / 0 = NaN and nothing reaches the logits: the gradient is taken as zero."""
    lg, y = ce_inputs(regime, C, M, ignore)

    def run(dt):
        l = lg.to(dt).requires_grad_(True)
        v = F.cross_entropy(l, y, ignore_index=IGNORE)
        if ignore == "all":
            return {"loss": v.detach(), "dlogits": torch.zeros_like(l)}
        v.backward()
        return {"loss": v.detach(), "dlogits": l.grad}
    return Ref(run)


def ce_loss_log1p64(lg, y):
    """The mean loss in float64 as log1p(rest) + (mx - l[y]), rest = the sum of exp(l[c] - mx) over every class but one maximal."""
    l = lg.double().numpy()
    keep = y.numpy() != IGNORE
    l, yy = l[keep], y.numpy()[keep]
    if len(yy) == 0:
        return float("nan")
    am = l.argmax(1)
    rows = np.arange(len(yy))
    mx = l[rows, am]
    e = np.exp(l - mx[:, None])
    e[rows, am] = 0.0
    return float(np.mean(np.log1p(e.sum(1)) + (mx - l[rows, yy])))


def _ce_rows32(lg, y):
    l = lg.numpy().astype(np.float32)
    keep = y.numpy() != IGNORE
    return l[keep], y.numpy()[keep], np.arange(int(keep.sum()))


def ce_loss_old_formula32(lg, y):
    """(mx + logf(se)) - l[y] in fp32 per pixel, summed in double: what the three kernel sites computed.  For the host test only."""
    l, yy, rows = _ce_rows32(lg, y)
    mx = l.max(1)
    se = np.zeros_like(mx)
    for c in range(l.shape[1]):
        se = (se + np.exp(l[:, c] - mx, dtype=np.float32)).astype(np.float32)
    term = ((mx + np.log(se, dtype=np.float32)).astype(np.float32) - l[rows, yy]).astype(np.float32)
    return float(np.float32(term.astype(np.float64).mean())) if len(yy) else float("nan")


def ce_loss_log1p_formula32(lg, y):
    """log1pf(rest) + (mx - l[y]) in fp32 per pixel, summed in double.  For the host test only."""
    l, yy, rows = _ce_rows32(lg, y)
    if not len(yy):
        return float("nan")
    am = l.argmax(1)
    mx = l[rows, am]
    rest = np.zeros_like(mx)
    for c in range(l.shape[1]):
        e = np.exp(l[:, c] - mx, dtype=np.float32)
        rest = np.where(am == c, rest, (rest + e).astype(np.float32))
    term = (np.log1p(rest, dtype=np.float32) + (mx - l[rows, yy]).astype(np.float32)).astype(np.float32)
    return float(np.float32(term.astype(np.float64).mean()))


# ---- validation loss (SegmentationEvaluator) ----------------------------------------------------------------------------------------
EVAL_BATCHES = ((2, 33, 35), (3, 16, 16), (1, 65, 63))       # as test_loss_matches_float64_and_is_reproducible: unequal, odd H * W
EVAL_DICE_SMOOTH = 1.0
# (loss, C, storage): "aligned" takes the C == 2 fast path, "offset1" the view of test_unaligned_storage_takes_the_generic_path
EVAL_PATHS = [("ce", 2, "aligned"), ("ce", 2, "offset1"), ("ce", 3, "aligned"), ("ce", 5, "aligned"), ("ce", 12, "aligned"),
              ("ce+dice", 2, "aligned"), ("ce+dice", 3, "aligned"), ("ce+dice", 5, "aligned"), ("ce+dice", 8, "aligned")]


def eval_inputs(regime, loss, C):
    """[(logits (b, H, W, C) fp32, labels (b, H, W))] of the three batches; every seventh pixel ignored for "ce" (F.one_hot of the
    dice loss takes no -100)."""
    out = []
    for b, H, W in EVAL_BATCHES:
        lg, y = ce_inputs(regime, C, b * H * W, "seventh" if loss == "ce" else "none")
        out.append((lg.view(b, H, W, C), y.view(b, H, W)))
    return out


def dice64(logits, y, smooth):
    """dice_loss of the reference training script, in the dtype of `logits` (B, C, H, W)."""
    pr = torch.softmax(logits, dim=1)
    oh = F.one_hot(y, num_classes=pr.shape[1]).permute(0, 3, 1, 2).to(logits.dtype)
    inter = (pr * oh).sum(dim=(2, 3))
    union = pr.sum(dim=(2, 3)) + oh.sum(dim=(2, 3))
    return 1.0 - ((2.0 * inter + smooth) / (union + smooth)).mean()


@lru_cache(maxsize=None)
def eval_reference(regime, loss, C) -> Ref:
    """The mean over the batches of each batch's loss, as SegmentationEvaluator.compute() reports it."""
    batches = eval_inputs(regime, loss, C)

    def run(dt):
        vs = []
        for lg, y in batches:
            l = lg.permute(0, 3, 1, 2).to(dt)
            v = F.cross_entropy(l, y, ignore_index=IGNORE)
            if loss == "ce+dice":
                v = v + dice64(l, y, EVAL_DICE_SMOOTH)
            vs.append(v.double())
        return {"loss": torch.stack(vs).mean()}
    return Ref(run)


# ---- Adam and SGD -------------------------------------------------------------------------------------------------------------------
OPT_GRID = 256 * 8 * 256           # launch_adam / launch_sgd: at most 256 * 8 workgroups of 256
OPT_SIZES = (1, 255, 257, 100003, OPT_GRID + 1)
OPT_STEPS = 3
ADAM_LR, ADAM_BETAS, ADAM_EPS = 1e-3, (0.9, 0.999), 1e-8


@lru_cache(maxsize=None)
def opt_cap() -> float:
    """test_adam_kernel_exact's 5e-7 on p, divided by the largest update of that test's case (its own float64 formula)."""
    n = 100003
    p, g, m, v = (torch.from_numpy(a).double() for a in (
        O.formula_normal("adam/p", (n,), seed=1), O.formula_normal("adam/g", (n,), seed=2) * np.float32(1e-2),
        O.formula_normal("adam/m", (n,), seed=3) * np.float32(1e-3), O.formula_uniform("adam/v", (n,), 0.0, 1e-4, seed=4)))
    lr, b1, b2, eps, wd, step, gs = 1e-3, 0.9, 0.999, 1e-8, 1e-4, 7, 0.5
    gt = g * gs + wd * p
    m2, v2 = b1 * m + (1 - b1) * gt, b2 * v + (1 - b2) * gt * gt
    upd = (lr / (1 - b1 ** step)) * m2 / (v2.sqrt() / np.sqrt(1 - b2 ** step) + eps)
    return ADAM_EXISTING_BAR / float(upd.abs().max())


# tag: (magnitudes, first step, state given, grad_scale, weight decay)
#   magnitudes "small": p ~ 1e-3 N, g ~ 1e-2 N, m ~ 3e-3 N, v ~ U(2e-5, 1e-4);  "existing": those of test_adam_kernel_exact;
#   "decay_only": the small p with g = 0
ADAM_CASES = {
    "small_s1": ("small", 1, False, 1.0, 1e-4),
    "small_s1000": ("small", 1000, True, 1.0, 1e-4),
    "small_s1_gs8_wd0": ("small", 1, False, 0.125, 0.0),
    "small_s1000_gs8": ("small", 1000, True, 0.125, 1e-4),
    "small_s1000_wd0": ("small", 1000, True, 1.0, 0.0),
    "existing_s7": ("existing", 7, True, 0.5, 1e-4),         # |p| up to 4.5: half an ulp of p is 2e-5 of the update, within CAP
    "small_s1e6": ("small", 10 ** 6, True, 1.0, 1e-4),       # both corrections are 1
    "decay_only": ("decay_only", 1, False, 1.0, 1e-4),       # g = 0 and v = 0: the weight decay is the whole gradient, 1e-7 ~ 10 eps
}
ADAM_SMALL = ("small_s1", "small_s1000")                     # the two chains of the write-up
ADAM_UNCHANGED = ("unchanged", 1, False, 1.0, 0.0)           # g = 0, zero state, no decay: p, m and v stay bit for bit
ADAM_RUNS = [("small_s1", n) for n in OPT_SIZES] + [(t, 100003) for t in ADAM_CASES if t != "small_s1"] + [("small_s1000", 257)]


def adam_inputs(tag, n):
    """(p, [g] * OPT_STEPS, m, v, first step, grad_scale, weight decay), fp32 tensors of n elements."""
    mag, step, given, gs, wd = ADAM_UNCHANGED if tag == "unchanged" else ADAM_CASES[tag]
    if mag == "existing":
        p = _normal("adam/p", (n,), 1)
        gr = [_normal("adam/g" if i == 0 else f"scase/adam/g{i}", (n,), 2) * 1e-2 for i in range(OPT_STEPS)]
        m = _normal("adam/m", (n,), 3) * 1e-3
        v = torch.from_numpy(O.formula_uniform("adam/v", (n,), 0.0, 1e-4, seed=4))
    else:
        p = _normal("scase/adam/p", (n,), 1) * 1e-3
        gr = [_normal(f"scase/adam/g{i}", (n,), 2) * (1e-2 if mag == "small" else 0.0) for i in range(OPT_STEPS)]
        m = _normal("scase/adam/m", (n,), 3) * 3e-3
        v = torch.from_numpy(O.formula_uniform("scase/adam/v", (n,), 2e-5, 1e-4, seed=4))
    if not given:
        m, v = torch.zeros(n), torch.zeros(n)
    return p.float(), [g.float() for g in gr], m.float(), v.float(), step, gs, wd


def _adam_chain(p, grads, m, v, step, gs, wd, dt):
    """torch.optim.Adam itself over the chain, its state set to (step - 1, m, v) first."""
    w = torch.nn.Parameter(p.to(dt).clone())
    opt = torch.optim.Adam([w], lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=wd, foreach=False)
    w.grad = torch.zeros_like(w)
    opt.step()                                               # creates the state in the layout this torch version uses
    st = opt.state[w]
    with torch.no_grad():
        w.copy_(p.to(dt))
        st["exp_avg"].copy_(m.to(dt))
        st["exp_avg_sq"].copy_(v.to(dt))
        if torch.is_tensor(st["step"]):
            st["step"].fill_(float(step - 1))
        else:
            st["step"] = step - 1
    for g in grads:
        w.grad = g.to(dt) * gs
        opt.step()
    return w.detach(), st["exp_avg"], st["exp_avg_sq"]


def update_of(p_after, p_start):
    """p_after - p_start in float64 (exact for fp32 operands)."""
    return LC._np64(p_after) - LC._np64(p_start)


@lru_cache(maxsize=None)
def adam_reference(tag, n) -> Ref:
    p, grads, m, v, step, gs, wd = adam_inputs(tag, n)

    def run(dt):
        w, m2, v2 = _adam_chain(p, grads, m, v, step, gs, wd, dt)
        return {"p": update_of(w, p), "m": m2, "v": v2}
    return Ref(run)


def adam_formula32(tag, n, corrections):
    """The kernel's per-element arithmetic in numpy fp32 over the chain, with 1 - beta and the two bias corrections formed as
    `corrections` says: "powf32" from fp32 betas, 1.f - beta and 1.f - powf(beta, step) (what launch_adam and the kernel did);
    "double" from the double betas on the host, cast once.  For the host test only.  Returns {"p": update, "m", "v"}."""
    f = np.float32
    p0, grads, m, v, step, gs, wd = adam_inputs(tag, n)
    p, m, v = p0.numpy().copy(), m.numpy().copy(), v.numpy().copy()
    lr, b1, b2, eps, wd, gs = f(ADAM_LR), f(ADAM_BETAS[0]), f(ADAM_BETAS[1]), f(ADAM_EPS), f(wd), f(gs)
    for k, g in enumerate(grads):
        s = step + k
        if corrections == "powf32":
            omb1, omb2 = f(1) - b1, f(1) - b2
            bc1 = f(1) - f(np.power(b1, f(s), dtype=f))
            bc2s = np.sqrt(f(1) - f(np.power(b2, f(s), dtype=f)), dtype=f)
        else:
            assert corrections == "double", corrections
            omb1, omb2 = f(1.0 - ADAM_BETAS[0]), f(1.0 - ADAM_BETAS[1])
            bc1 = f(1.0 - ADAM_BETAS[0] ** s)
            bc2s = f(np.sqrt(1.0 - ADAM_BETAS[1] ** s))
        gi = g.numpy() * gs + wd * p
        m = b1 * m + omb1 * gi
        v = b2 * v + omb2 * gi * gi
        p = p - (lr / bc1) * m / (np.sqrt(v) / bc2s + eps)
        assert p.dtype == f and m.dtype == f and v.dtype == f
    return {"p": update_of(p, p0), "m": m, "v": v}


SGD_LR = 1e-2
SGD_CASES = {f"m{mom}_wd{wd}": (mom, wd) for mom in (0.0, 0.9) for wd in (0.0, 1e-4)}
SGD_RUNS = [("m0.9_wd0.0001", n) for n in OPT_SIZES] + [(t, 100003) for t in SGD_CASES if t != "m0.9_wd0.0001"]


def sgd_inputs(tag, n):
    """(p, [g] * OPT_STEPS, momentum, weight decay): the small weights of the Adam cases, so that rounding p cannot reach the bar."""
    mom, wd = SGD_CASES[tag]
    p = _normal("scase/sgd/p", (n,), 1) * 1e-3
    return p.float(), [(_normal(f"scase/sgd/g{i}", (n,), 2) * 1e-2).float() for i in range(OPT_STEPS)], mom, wd


@lru_cache(maxsize=None)
def sgd_reference(tag, n) -> Ref:
    p, grads, mom, wd = sgd_inputs(tag, n)

    def run(dt):
        w = torch.nn.Parameter(p.to(dt).clone())
        opt = torch.optim.SGD([w], lr=SGD_LR, momentum=mom, weight_decay=wd, foreach=False)
        for g in grads:
            w.grad = g.to(dt)
            opt.step()
        out = {"p": update_of(w.detach(), p)}
        if mom:
            out["buf"] = opt.state[w]["momentum_buffer"]
        return out
    return Ref(run)
