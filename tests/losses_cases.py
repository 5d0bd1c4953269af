"""Deterministic cases, float64 references and error bars for the auxiliary-loss kernels (csrc/losses.hip: TV, dice, feature
consistency, elliptical shape) and FeatureFusion's two kernels (csrc/imageops.hip: bilinear resize, region-map gather).  Plain
torch / numpy on the CPU, inputs from the oracle's formula tensors: no fixture, no GPU.  Imported by
tests/test_losses_cases_host.py (case properties, closed forms, no GPU) and tests/test_gpu_losses_f64.py (the kernels).

The bars.  The reference is the oracle run in float64 under autograd.  `cond` is the deviation of the SAME oracle code run in
fp32 from that, i.e. the reference's own arithmetic error on the case:

    value      |v32 - v64| / max(1, |v64|)
    tensor     max|g32 - g64| / max|g64|        (gradients, the resized map)
    bar        4 * cond + 2^-22, and never above the bar the fixture tests already hold for the quantity (CAP)

4: the kernels do the fp32 oracle's per-element arithmetic in another order and with expf, and sum in double; a wrong term,
class, divisor or stride errs by 1e-3 or more.  2^-22 (2.4e-7): the floor for a case on which the fp32 oracle lands exactly.
Where the float64 gradient is identically zero the kernel's has to be exactly zero.  The shape loss is double arithmetic cast to
float: |got - ref64| <= 5e-7 * max(1, |ref64|) (6e-8 for the cast, the rest for the one-pass moments)."""
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

import mgunet_oracle as O

FLOOR = 2.0 ** -22
SHAPE_BAR = 5e-7
# the bars of tests/test_gpu_losses_pipeline.py for the same quantities: no bar here exceeds them
CAP = {"value": 2e-6, "tv": 2e-6, "dice": 5e-6, "featcons": 1e-5, "resize": 2e-6}


def _np64(t):
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)


def err_of(name: str, got, ref64) -> float:
    """The measure of the module docstring: `value` is a scalar with a floor of 1 in the denominator, anything else a tensor
    measured against its largest reference element (0 / inf where the reference is identically zero and got is / is not)."""
    g, r = _np64(got), _np64(ref64)
    assert g.shape == r.shape, (name, g.shape, r.shape)
    d = float(np.abs(g - r).max())
    if not np.isfinite(d):
        return float("inf")
    if name == "value":
        return d / max(1.0, abs(float(r)))
    m = float(np.abs(r).max())
    if m == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / m


class Ref:
    """run(dtype) -> {name: tensor}; keeps the float64 results and cond of each from the fp32 run of the same code."""
    measure = staticmethod(err_of)   # a subclass may measure a quantity another way (tests/step_cases.py: a loss relative to itself)

    def __init__(self, run):
        r64, r32 = run(torch.float64), run(torch.float32)
        self.r64 = {k: _np64(v) for k, v in r64.items()}
        self.cond = {k: self.measure(k, r32[k], self.r64[k]) for k in r64}

    def bar(self, name: str, cap: float) -> float:
        return min(4.0 * self.cond[name] + FLOOR, cap)

    def check(self, name: str, got, cap: float, what: str) -> float:
        """Print the NOTES.md table row, then assert got within the bar of the float64 reference `name`."""
        err, bar = self.measure(name, got, self.r64[name]), self.bar(name, cap)
        print(f"| {what} | {name} | {self.cond[name]:.1e} | {bar:.1e} | {err:.1e} |")
        assert err <= bar, (what, name, "err", err, "bar", bar, "cond", self.cond[name])
        return err


def autograd_run(fn, leaves, dt, post=None, needs=None, names=None):
    """fn(*leaves in dt) -> scalar v; backward of post(v) (default v itself).  {"value": v, names[i]: d post(v) / d leaf i}."""
    needs = needs or (True,) * len(leaves)
    ls = [t.to(dt).requires_grad_(n) for t, n in zip(leaves, needs)]
    v = fn(*ls)
    (post(v) if post else v).backward()
    out = {"value": v.detach()}
    for t, n, k in zip(ls, needs, names):
        if n:
            out[k] = t.grad
    return out


# ---- storage layouts of one logical (B, C, H, W) tensor -----------------------------------------------------------------------------
def _filler(name, shape, like):
    return torch.from_numpy(O.formula_normal("lcase/fill/" + name, shape, seed=7)).to(device=like.device, dtype=like.dtype)


def lay_nchw(x):
    return x.contiguous()


def lay_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def lay_chslice(x):
    """Channels [1, 1 + C) of a (C + 2)-channel NHWC-stored tensor (x[:, 1:4] for C = 3)."""
    B, C, H, W = x.shape
    wide = lay_nhwc(_filler("chslice", (B, C + 2, H, W), x))
    wide[:, 1:1 + C] = x
    return wide[:, 1:1 + C]


def lay_first_of_8(x):
    """Channels [0, C) of an 8-channel NHWC-stored tensor (the trainer's padded logits)."""
    B, C, H, W = x.shape
    wide = lay_nhwc(_filler("of8", (B, 8, H, W), x))
    wide[:, :C] = x
    return wide[:, :C]


def lay_crop(x):
    """big[:, :, 1:-1, 2:-3] of a contiguous (B, C, H + 2, W + 5) tensor."""
    B, C, H, W = x.shape
    big = _filler("crop", (B, C, H + 2, W + 5), x).contiguous()
    big[:, :, 1:-1, 2:-3] = x
    return big[:, :, 1:-1, 2:-3]


# ---- total variation ----------------------------------------------------------------------------------------------------------------
TV_WEIGHT, TV_UP = 0.7, 3.0
TV_BIG = (4, 1, 512, 513)          # 1 050 624 elements: just over 1024 workgroups of 1024
TV_SHAPES = [(1, 1, 2, 2), (2, 3, 2, 37), (3, 2, 41, 2), (2, 5, 17, 23), TV_BIG]
TV_LAYOUTS = {"nchw": lay_nchw, "nhwc": lay_nhwc, "chslice": lay_chslice, "crop": lay_crop}
TV_CHAINED = (2, 5, 17, 23)        # also run with post(v) = TV_UP * v + v^2 / 2: grad_output = TV_UP + v, a device scalar


def tv_layouts(shape):
    return ["nchw"] if shape == TV_BIG else list(TV_LAYOUTS)


def tv_input(shape):
    return torch.from_numpy(O.formula_normal("lcase/tv/x", shape, seed=shape[2]))


def tv_post(chained):
    return (lambda v: TV_UP * v + 0.5 * v * v) if chained else (lambda v: TV_UP * v)


@lru_cache(maxsize=None)
def tv_reference(shape, chained=False) -> Ref:
    x = tv_input(shape)
    return Ref(lambda dt: autograd_run(lambda a: O.tv_loss(a, TV_WEIGHT), [x], dt, tv_post(chained), names=["dx"]))


# ---- dice ---------------------------------------------------------------------------------------------------------------------------
# tag: (B, C, H, W, logit scale, smooth)
DICE_CASES = {f"c{C}": (2, C, 19, 23, 2.0, 1.0) for C in range(1, 9)}
DICE_CASES["cap"] = (1, 7, 363, 363, 3.0, 1.0)      # HW = 131 769 > 128 workgroups of 1024
DICE_CASES["absent"] = (3, 4, 19, 23, 3.0, 1e-3)    # class 2 absent from the batch, class 3 from image 1
DICE_CASES["saturated"] = (2, 5, 19, 23, 60.0, 1.0)
DICE_CASES["h1"] = (2, 3, 1, 37, 2.0, 1.0)          # one row, one column: the wrapper's one-pixel-stride test with a size-1 dimension
DICE_CASES["w1"] = (2, 3, 41, 1, 2.0, 1.0)
DICE_LAYOUTS = {"nchw": lay_nchw, "nhwc": lay_nhwc, "first_of_8": lay_first_of_8, "crop": lay_crop}
DICE_RAW = ("c3", "c6")
DICE_RAW_PITCH, DICE_RAW_SCALE, DICE_RAW_SCALE_DEV, DICE_RAW_PREFILL = 8, 0.5, 1.75, 1e-4


def dice_inputs(tag):
    B, C, H, W, scale, smooth = DICE_CASES[tag]
    lg = torch.from_numpy(O.formula_normal(f"lcase/dice/{tag}/l", (B, C, H, W), seed=C)) * scale
    y = torch.from_numpy(O.formula_labels(f"lcase/dice/{tag}/y", (B, H, W), C, seed=C + 1)).clone()
    if tag == "absent":
        y[y == 2] = 0
        y[1][y[1] == 3] = 1
    return lg, y, smooth


@lru_cache(maxsize=None)
def dice_reference(tag) -> Ref:
    lg, y, smooth = dice_inputs(tag)
    return Ref(lambda dt: autograd_run(lambda l: O.dice_loss(l, y, smooth), [lg], dt, names=["dlogits"]))


def dice_closed_form(lg, y, smooth):
    """dL/dlogits in float64 as the comment above dice_coef_kernel states it: dL/dI = -2 / (B C U), dL/dP = (2 I + s) / (B C U^2),
    U = P + T + s, q_c = dL/dI [y == c] + dL/dP, dlogit_k = p_k (q_k - sum_c q_c p_c)."""
    B, C, H, W = lg.shape
    p = torch.softmax(lg.double(), dim=1)
    oh = F.one_hot(y, C).permute(0, 3, 1, 2).double()
    I, P, T = (p * oh).sum((2, 3)), p.sum((2, 3)), oh.sum((2, 3))
    U = P + T + smooth
    dI, dP = -2.0 / (B * C * U), (2.0 * I + smooth) / (B * C * U * U)
    q = dI[:, :, None, None] * oh + dP[:, :, None, None]
    return p * (q - (q * p).sum(1, keepdim=True))


def dice_raw_prefill(tag):
    """(B * HW, 8) fp32 destination values of the gradient's own magnitude, so that the accumulate check bites."""
    B, C, H, W, _, _ = DICE_CASES[tag]
    return torch.from_numpy(O.formula_normal(f"lcase/dice/{tag}/pre", (B * H * W, DICE_RAW_PITCH), seed=3)) * DICE_RAW_PREFILL


@lru_cache(maxsize=None)
def dice_raw_reference(tag) -> Ref:
    """Columns [0, C) after the accumulating call: prefill + grad_scale * (*grad_scale_dev) * dL/dlogits, rows = pixels."""
    B, C, H, W, _, _ = DICE_CASES[tag]
    lg, y, smooth = dice_inputs(tag)
    pre = dice_raw_prefill(tag)[:, :C]
    k = DICE_RAW_SCALE * DICE_RAW_SCALE_DEV

    def run(dt):
        r = autograd_run(lambda l: O.dice_loss(l, y, smooth), [lg], dt, names=["g"])
        return {"acc": pre.to(dt) + k * r["g"].permute(0, 2, 3, 1).reshape(B * H * W, C)}
    return Ref(run)


# ---- feature consistency ------------------------------------------------------------------------------------------------------------
# tag: (B, N, D, margin rule, y rule, coincident row's y or None, (d f_unet wanted, d f_graph wanted))
#   margin rule: a number, or "below" / "above" every row's distance;  y rule: "hard" {0, 1} or "soft" = 0.3 * labels + 0.2
FEATCONS_UP = 3.0
FEATCONS_CASES = {}
for _i, _D in enumerate((4, 20, 64, 68, 132)):        # one live lane, a part trip, a full trip, a second trip, a third
    for _j, (_B, _N) in enumerate(((1, 1), (2, 5), (3, 130))):
        # the lone row of (1, 1) gets margin 1.0: at 0.7 its hinge margin - dist would be a cancellation, and the case ill-conditioned
        FEATCONS_CASES[f"d{_D}_{_B}x{_N}"] = (_B, _N, _D, 1.0 if _N == 1 else 0.7, "hard", None if _N == 1 else (_i + _j) % 2,
                                              (True, True))
FEATCONS_CASES["n4100"] = (2, 4100, 64, 0.7, "hard", 0, (True, True))
FEATCONS_CASES["cap"] = (1, 66000, 4, 0.7, "hard", 1, (True, True))         # rows > 65 536: the grid-stride loop
FEATCONS_CASES["soft"] = (2, 37, 68, 0.7, "soft", None, (True, True))
FEATCONS_CASES["coincident_y0"] = (2, 5, 20, 0.7, "hard", 0, (True, True))
FEATCONS_CASES["coincident_y1"] = (2, 5, 20, 0.7, "hard", 1, (True, True))
FEATCONS_CASES["margin_below"] = (3, 50, 68, "below", "hard", None, (True, True))
FEATCONS_CASES["margin_above"] = (3, 50, 68, "above", "hard", None, (True, True))
FEATCONS_CASES["only_unet"] = (3, 130, 68, 0.7, "hard", 0, (True, False))
FEATCONS_CASES["only_graph"] = (3, 130, 68, 0.7, "hard", 1, (False, True))


def featcons_distances(fu, fg):
    return torch.sqrt(((fu.double() - fg.double()) ** 2).sum(2) + 1e-8)


def featcons_inputs(tag):
    """(f_unet, f_graph, y fp32 (B, N), margin, needs).  Distances are about 0.7 (+- 0.7 / sqrt(2 D))."""
    B, N, D, mrule, yrule, coin, needs = FEATCONS_CASES[tag]
    s = 0.7 / float(np.sqrt(D))
    fu = torch.from_numpy(O.formula_normal(f"lcase/fc/{tag}/u", (B, N, D), seed=D)) * s
    fg = fu + torch.from_numpy(O.formula_normal(f"lcase/fc/{tag}/g", (B, N, D), seed=D + 1)) * s
    y = torch.from_numpy(O.formula_labels(f"lcase/fc/{tag}/y", (B, N), 2, seed=D + 2)).float()
    if yrule == "soft":
        y = 0.3 * y + 0.2
    if coin is not None:
        fg[0, 0] = fu[0, 0]
        y[0, 0] = float(coin)
    dist = featcons_distances(fu, fg)
    margin = {"below": 0.5 * float(dist.min()), "above": 2.0 * float(dist.max())}.get(mrule, mrule)
    return fu, fg, y, float(margin), needs


@lru_cache(maxsize=None)
def featcons_reference(tag) -> Ref:
    fu, fg, y, margin, needs = featcons_inputs(tag)
    return Ref(lambda dt: autograd_run(lambda a, b: O.feature_consistency_loss(a, b, y, margin), [fu, fg], dt,
                                       lambda v: FEATCONS_UP * v, needs, ["dfu", "dfg"]))


# ---- elliptical shape: masks form ---------------------------------------------------------------------------------------------------
SHAPE_EPS = 1e-6
SHAPE_HW = 24
SHAPE_SPECIAL = ["full", "borders", "px9", "px10", "row12", "diag12", "diag13", "empty"]   # objects 62 .. 69
SHAPE_COUNT = 70                                 # shape_params_kernel: 64 objects per workgroup, 64 .. 69 in the second
SHAPE_BIG_HW = 520                               # HW = 270 400 > 256 workgroups of 1024


def ellipse_mask(H, W, cy, cx, a, b, theta):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u = (xx - cx) * np.cos(theta) + (yy - cy) * np.sin(theta)
    v = -(xx - cx) * np.sin(theta) + (yy - cy) * np.cos(theta)
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


def shape_special(name):
    n = SHAPE_HW
    m = np.zeros((n, n), dtype=bool)
    if name == "full":
        m[:] = True
    elif name == "borders":                      # a two-pixel frame: touches all four borders
        m[:2], m[-2:], m[:, :2], m[:, -2:] = True, True, True, True
    elif name in ("px9", "px10"):                # a 3 x 3 blob: skipped; with a tenth pixel: kept
        m[5:8, 9:12] = True
        m[8, 9] = name == "px10"
    elif name == "row12":
        m[7, 3:15] = True
    elif name in ("diag12", "diag13"):
        m[np.arange(4, 16), np.arange(6, 18)] = True
        m[4, 7] = name == "diag13"
    return m


@lru_cache(maxsize=None)
def shape_masks():
    """The 70 objects of the 24 x 24 call as a bool array (70, 24, 24): 62 ellipses at varied orientations, then SHAPE_SPECIAL."""
    k = SHAPE_COUNT - len(SHAPE_SPECIAL)
    u = O.formula_uniform("lcase/shape/ell", (k, 4), 0.0, 1.0, 1).astype(np.float64)
    out = [ellipse_mask(SHAPE_HW, SHAPE_HW, 9.0 + 6.0 * u[i, 0], 9.0 + 6.0 * u[i, 1], 4.0 + 6.0 * u[i, 2], 2.0 + 3.0 * u[i, 3],
                        np.pi * i / k) for i in range(k)]
    return np.stack(out + [shape_special(s) for s in SHAPE_SPECIAL])


@lru_cache(maxsize=None)
def shape_big_masks():
    """(2, 520, 520): a 200 x 120 ellipse turned by 0.5 rad, and a band 2.4 pixels thick of slope 1 / 2 from border to border."""
    n = SHAPE_BIG_HW
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    band = np.abs((yy - 260.0) - 0.5 * (xx - 260.0)) <= 1.2
    return np.stack([ellipse_mask(n, n, 255.0, 262.0, 200.0, 120.0, 0.5), band])


def shape_reference(masks) -> float:
    """The float64 oracle over a list / array of (H, W) bool masks."""
    return float(O.elliptical_shape_loss(None, [[torch.from_numpy(np.ascontiguousarray(m)) for m in masks]], SHAPE_EPS,
                                         dtype=torch.float64))


def shape_term_raw_moments(mask, eps=SHAPE_EPS):
    """One object's term restated in one pass over raw moments (the kernels' route), float64 numpy; None if under 10 pixels."""
    ys, xs = np.nonzero(mask)
    n = float(len(ys))
    if n < 10:
        return None
    ys, xs = ys.astype(np.float64), xs.astype(np.float64)
    cy, cx = ys.sum() / n, xs.sum() / n
    syy = ((ys * ys).sum() - n * cy * cy) / (n - 1) + eps
    sxy = ((ys * xs).sum() - n * cy * cx) / (n - 1)
    sxx = ((xs * xs).sum() - n * cx * cx) / (n - 1) + eps
    det = syy * sxx - sxy * sxy
    i00, i01, i11 = sxx / det, -sxy / det, syy / det
    y, x = ys - cy, xs - cx
    mah = y * (i00 * y + i01 * x) + x * (i01 * y + i11 * x)
    return float(((mah - 1.0) ** 2).sum() / n)


def shape_loss_raw_moments(masks) -> float:
    terms = [t for t in (shape_term_raw_moments(m) for m in masks) if t is not None]
    return sum(terms) / len(terms) if terms else 0.0


# ---- elliptical shape: probabilities form -------------------------------------------------------------------------------------------
PROBS_CLASSES = (2, 3, 5)
PROBS_B, PROBS_H, PROBS_W = 3, 24, 31
TIE_01 = (slice(1, 3), slice(26, 30))            # image 0: class 0 == class 1 on top -> arg-max 0, not foreground
TIE_12 = (slice(20, 23), slice(1, 4))            # image 0, C >= 3: class 1 == class 2 on top -> arg-max 1, foreground


def probs_input(C):
    """(3, C, 24, 31) fp32 scores in [0, 1].  Image 0: an ellipse of class 1 plus the two tie blocks, far from the ellipse so that
    either tie read the other way moves the loss; image 1: 7 foreground pixels (skipped, leaves the denominator); image 2: another
    ellipse.  Elsewhere class 0, or for C >= 3 a higher class on a fifth of the pixels, is on top."""
    B, H, W = PROBS_B, PROBS_H, PROBS_W
    p = torch.from_numpy(O.formula_uniform(f"lcase/probs/{C}", (B, C, H, W), 0.0, 0.4, seed=C)).clone()
    other = torch.from_numpy(O.formula_labels(f"lcase/probs/{C}/o", (B, H, W), 5, seed=C + 1)) == 0
    fg = np.zeros((B, H, W), dtype=bool)
    fg[0] = ellipse_mask(H, W, 11.0, 13.0, 9.0, 5.0, 0.4)
    fg[1, 3, 4:11] = True
    fg[2] = ellipse_mask(H, W, 13.0, 17.0, 11.0, 6.0, 2.0)
    fg = torch.from_numpy(fg)
    for b in range(B):
        p[b, 0][~fg[b]] = 0.8
        if C >= 3:
            p[b, C - 1][~fg[b] & other[b]] = 0.85
        p[b, 1][fg[b]] = 0.9
    p[0, :, TIE_01[0], TIE_01[1]] = 0.1
    p[0, 0:2, TIE_01[0], TIE_01[1]] = 0.95
    if C >= 3:
        p[0, :, TIE_12[0], TIE_12[1]] = 0.1
        p[0, 1:3, TIE_12[0], TIE_12[1]] = 0.95
    return p


def probs_reference(p) -> float:
    return float(O.elliptical_shape_loss(p, None, SHAPE_EPS, dtype=torch.float64))


@lru_cache(maxsize=None)
def probs_case_reference(C) -> float:
    return probs_reference(probs_input(C))


# ---- FeatureFusion: bilinear resize -------------------------------------------------------------------------------------------------
RESIZE_SIZES = [((5, 7), (13, 18)), ((37, 45), (8, 10)), ((1, 9), (4, 20)), ((9, 1), (20, 4)), ((12, 20), (1, 1)),
                ((12, 20), (24, 40))]
RESIZE_CHANNELS = (4, 36)
RESIZE_B = 2
RESIZE_LD, RESIZE_OFF, SENTINEL = 48, 8, -77.25


def resize_input(src, C):
    return torch.from_numpy(O.formula_normal("lcase/resize/x", (RESIZE_B, C) + tuple(src), seed=C + src[0]))


@lru_cache(maxsize=None)
def resize_reference(src, dst, C) -> Ref:
    x = resize_input(src, C)
    return Ref(lambda dt: {"map": F.interpolate(x.to(dt), size=dst, mode="bilinear", align_corners=False)})


# ---- FeatureFusion: region-map gather -----------------------------------------------------------------------------------------------
GATHER_R = 7
GATHER_DIMS = (4, 12)
GATHER_B, GATHER_H, GATHER_W = 2, 5, 9
GATHER_LD, GATHER_OFF = 24, 8
GATHER_PLANTED = [-1, 0, GATHER_R - 1, GATHER_R, GATHER_R + 5, 2 ** 31 + 1]     # 2^31 + 1 is 1 to a kernel that truncates to int


def gather_inputs(D):
    """(table (R, D) fp32, ids (B, H, W) int64): random ids inside [0, R), the planted ones at the start of each image."""
    table = torch.from_numpy(O.formula_normal("lcase/gather/t", (GATHER_R, D), seed=D))
    ids = torch.from_numpy(O.formula_labels("lcase/gather/i", (GATHER_B, GATHER_H, GATHER_W), GATHER_R, seed=D + 1)).clone()
    for b in range(GATHER_B):
        ids[b].view(-1)[:len(GATHER_PLANTED)] = torch.tensor(GATHER_PLANTED)
    return table, ids


def gather_reference(table, ids):
    """(B, H, W, D): the table row of a valid id, zeros otherwise."""
    ok = (ids >= 0) & (ids < table.shape[0])
    out = table[torch.where(ok, ids, torch.zeros_like(ids))]
    out[~ok] = 0.0
    return out
