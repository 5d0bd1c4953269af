"""Host restatement of the fp32 eval forward, kernel form by kernel form, for tests/test_fp32_forms_host.py (CPU) and
tests/test_gpu_fp32_layers.py (GPU).  Everything that does not depend on the storage type is bf16_oracle's (segment, sources,
segment_names, the weight patterns of exact_params, exact_input, the indexing mutants), run here with Storage FP32.

The shape matrix.  CASES maps a case to (cfg = (in_channels, classes, init_features, depth), the (form, Cin, Cout) the case is there
for).  layer_forms(cfg, shape, switches) derives, the way pick_conv / wino_asm_shape / wino_head_layer / first_conv_applicable /
first_mfma_applicable / convt_x3_layer (csrc/igemm.hip, elementwise.hip, first_mfma.hip) and mgu_unet_forward (csrc/mgunet_api.hip)
decide, the launches of one fp32 eval forward with a patch-mean request at patch 16, in order; family_launches(...) counts them by
profiling-record name (conv_kernel_name and the ProfScope labels of mgu_unet_forward).

The bars (a) on formula weights, against the float64 segment computed from the path's own exposed predecessors:
  conv segments   |got - ref| <= L * c * S per element.  L = convolutions of the segment (2; 3 with a ConvTranspose; 5 through the
                  bottleneck).  S = the same segment in float64 on absolute values (|x|, |w|, |scale|, |shift|; ReLU is the identity
                  there): the propagated sum |a b|.  c = max(2e-6, 4 * worst |emulation - ref| / S of two CPU fp32 evaluations of the
                  segment: the library-order direct convolution and an F(2x2,3x3) Winograd with fp32 transforms).  2e-6 is the project's
                  per-layer Winograd bar relative to sum |a b| (tests/test_gpu_backward_kernels.py), 4 its `4 * cond` convention
                  (tests/step_cases.py).  c never sees a kernel.
  logits          <= C * 2^-24 * (sum |w f| + |b|): C fp32 products summed in any order, each rounding at most 2^-24 of the running sum.
  patch means     <= 255 * 2^-24 * mean |f| over the zero-padded 16 x 16 patch: 256 terms in any order.  A pixel taken from the wrong
                  patch moves a mean by about |f| / 256, some 250 times the bound.
(b) exact data: exact_params / exact_input with running_var = float32(1) - float32(1e-5), for which fl(var + 1e-5f) == 1.0f, so the
folded scale is exactly 1 and the shift exactly 0.  The float64 network with eps = 1 - var gives the one right answer (exact_reference).

Why the fp32 forward is exact on that data.  Inputs are integers 0..3; 3x3 weights are -1 / 0 / +1 with at most NNZ nonzeros per
output channel, ConvTranspose weights small integers, biases small integers: every activation is an integer below 256 (nnz_of keeps
it there; bf16_oracle's own exactness needs the same).  Direct kernels: integer products, partial sums below 2^24 in any order.
Winograd F(2x2,3x3): the input transform B^T d B adds and subtracts four integers (|V| <= 1020, 11 bits); the weight transform
G g G^T has entries that are multiples of 1/4 with |U| <= 9/4, at most 4 significant bits; a three-piece bf16 split of a value of
<= 24 significant bits is exact (3 x 8 bits), so each piece product is exact and so is every sum of them: in units of 1/4 the
element-wise products summed over <= 384 channels stay below 384 * 1020 * 9 < 2^22; the output transform A^T m A adds nine such
terms, still below 2^24 quarter-units, and the result is the integer the direct sum gives.  Scale 1, shift 0, ReLU and max keep
integers.  The head is a dense -1 / 0 / +1 row on integers below 256 (C <= 96: below 2^15); a patch sum is at most 256 * 255 < 2^16
and the division by 256 exact."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import bf16_oracle as B
import mgunet_oracle as O
from bf16_oracle import F64, FP32, _stride, exact_input, exact_seeds, nnz_of, segment_names, sources  # noqa: F401  (shared, not copied)

PATCH = 16
C_FLOOR = 2e-6          # the project's per-layer Winograd bar relative to sum |a b|
C_FACTOR = 4.0          # the project's `4 * cond` convention

# ---- the shape matrix -------------------------------------------------------------------------------------------------------------
# Forms: first_mfma, first_valu, tiles (igemm_kernel<f32>), wino_cp1 / wino_cp2 (the C++ component-pair kernels, narrow / wide),
# wino_asm_wide / wino_asm_cp1r2 / wino_asm_cp1r4 / wino_asm_cp1r2_head (their assembly forms), halo (conv3x3_halo_kernel<f32>),
# convt_x3, convt_generic; the non-conv passes maxpool2, head (conv1x1_head_kernel), patch_mean (patch_mean_kernel<float, 0>),
# patch_mean_head (patch_mean_kernel<float, NC>: C / 4 a power of two), patch_sum_combine.  A form followed by "+pool" fuses MaxPool.
CASES = {
    "f24d2": ((3, 2, 24, 2), [("tiles", 3, 24), ("tiles", 24, 24), ("tiles", 24, 48), ("wino_cp2+pool", 48, 48), ("wino_cp2", 48, 96),
                              ("wino_cp2", 96, 96), ("convt_generic", 96, 48), ("convt_generic", 48, 24), ("wino_cp1", 48, 24),
                              ("maxpool2", 24, 24), ("head", 24, 2), ("patch_mean", 24, 24)]),
    "f80d1": ((3, 2, 80, 1), [("wino_cp2+pool", 80, 80), ("wino_cp2", 80, 160), ("wino_cp2", 160, 160), ("wino_cp2", 160, 80),
                              ("convt_generic", 160, 80), ("head", 80, 2), ("patch_mean", 80, 80)]),
    "f96d1": ((3, 3, 96, 1), [("wino_cp2+pool", 96, 96), ("wino_cp2", 96, 192), ("wino_cp2", 192, 192), ("wino_asm_wide", 96, 192),
                              ("wino_asm_wide", 192, 192), ("convt_x3", 192, 96), ("head", 96, 3), ("patch_mean", 96, 96)]),
    "f64d1": ((3, 2, 64, 1), [("first_valu", 3, 64), ("wino_cp2+pool", 64, 64), ("wino_asm_wide+pool", 64, 64), ("convt_x3", 128, 64),
                              ("wino_asm_wide", 128, 64), ("wino_cp2", 128, 128), ("patch_mean_head", 64, 2)]),
    "f16d2": ((2, 3, 16, 2), [("first_valu", 2, 16), ("wino_cp1+pool", 16, 16), ("wino_cp1", 16, 32), ("convt_x3", 64, 32),
                              ("convt_generic", 32, 16), ("patch_mean_head", 16, 3)]),
    "f32d1c4": ((4, 4, 32, 1), [("first_valu", 4, 32), ("wino_asm_cp1r2+pool", 32, 32), ("wino_asm_cp1r4", 64, 32),
                                ("wino_asm_cp1r2_head", 32, 32), ("patch_sum_combine", 32, 32), ("patch_mean_head", 32, 4)]),
    "f32d3c1": ((1, 1, 32, 3), [("first_mfma", 1, 32), ("wino_cp1+pool", 32, 32), ("wino_cp2+pool", 64, 64), ("wino_cp2+pool", 128, 128),
                                ("wino_asm_cp1r2_head", 32, 32), ("patch_mean_head", 32, 1)]),
    "f24d1c4": ((4, 4, 24, 1), [("tiles", 4, 24), ("head", 24, 4), ("patch_mean", 24, 24), ("wino_cp1", 48, 24)]),
    "f48d1c1": ((3, 1, 48, 1), [("tiles", 3, 48), ("wino_cp2+pool", 48, 48), ("convt_generic", 96, 48), ("head", 48, 1), ("patch_mean", 48, 48)]),
    "f96d1_direct": ((3, 3, 96, 1), [("halo+pool", 96, 96), ("halo", 96, 192), ("halo", 192, 192), ("halo", 192, 96), ("tiles", 3, 96),
                                     ("convt_x3", 192, 96)]),
}
SWITCHES = {"f96d1_direct": {"MGU_NO_WINOGRAD": "1"}}       # set around context creation only

RECORD = {"first_mfma": "conv3x3_first_mfma_kernel", "first_valu": "conv3x3_first_kernel", "tiles": "igemm_kernel<f32>",
          "wino_cp1": "wino3x3_cp_kernel<1>", "wino_cp2": "wino3x3_cp_kernel<2>",
          "wino_asm_wide": "mgu_wino_cp2_gfx950 (asm form of wino3x3_cp_kernel<2>)",
          "wino_asm_cp1r2": "mgu_wino_cp1r2_gfx950 (asm form of wino3x3_cp_kernel<1>)",
          "wino_asm_cp1r4": "mgu_wino_cp1r4_gfx950 (asm form of wino3x3_cp_kernel<1>)",
          "wino_asm_cp1r2_head": "mgu_wino_cp1r2h_gfx950 (asm form of wino3x3_cp_kernel<1, head>: + 1x1 head + patch sums)",
          "halo": "conv3x3_halo_kernel<f32>", "convt_x3": "convt2x2_x3_kernel", "convt_generic": "igemm_kernel<f32> (ConvTranspose)",
          "maxpool2": "maxpool2", "head": "conv1x1_head_kernel", "patch_mean": "patch_mean_kernel",
          "patch_mean_head": "patch_mean_kernel (1x1 head + patch means)", "patch_sum_combine": "patch_sum_combine_kernel"}


def sizes(case):
    """small: below one patch; ragged: odd levels, odd-size concat, nothing eligible for assembly; whole: H % 16 == 0 and W % 32 == 0 on
    the first level (64 x 128 where the case wants the assembly wide kernel one level down: W / 2 % 32 == 0 as well)."""
    cin, depth = CASES[case][0][0], CASES[case][0][3]
    out = {"small": (2, cin, 12, 20), "ragged": (2, cin, 50, 70), "whole": (1, cin, 64, 128 if case == "f96d1" else 96)}
    if depth > 2:           # 12 x 20 leaves 1 x 2 at the bottleneck of a depth-3 network
        del out["small"]
    return out


def _conv_form(cp, n, h, w, ldout, coff, pool, head, sw):
    """pick_conv on a 3x3 fp32 layer (ldin == Cp everywhere in the network walk): (form, pool fused)."""
    wino = not sw.get("MGU_NO_WINOGRAD") and cp % 16 == 0
    if not wino:
        return ("halo", pool) if cp % 32 == 0 else ("tiles", False)
    wide = n > 32

    def asm_shape(with_pool):            # wino_asm_shape
        if wide and n % 64:
            return False
        if not wide and (n != 32 or cp not in (32, 64)):
            return False
        if h % 8 or w % 32 or cp % 32 or ldout % 4 or coff % 4:
            return False
        return not (with_pool and (h % 2 or w % 2))

    if head and asm_shape(pool) and not wide and not pool and ldout == 32 and coff == 0:
        return "wino_asm_cp1r2_head", pool
    if asm_shape(pool):
        return ("wino_asm_wide" if wide else "wino_asm_cp1r2" if cp == 32 else "wino_asm_cp1r4"), pool
    return ("wino_cp2" if wide else "wino_cp1"), pool


def layer_forms(cfg, shape, switches=None):
    """(form, Cin, Cout) of every launch of one fp32 eval forward of `shape` with a patch-mean request at patch 16, in launch order
    ("+pool": the MaxPool rides in the epilogue)."""
    sw = switches or {}
    cin0, ncls, f, depth = cfg
    Bn, _, H, W = shape
    hs, ws = [H], [W]
    for _ in range(depth):
        hs.append(hs[-1] // 2)
        ws.append(ws[-1] // 2)
    head_wanted = f == 32 and 1 <= ncls <= 4 and H % 16 == 0 and W % 32 == 0       # wino_head_layer (MGU_HEAD_FUSED default)
    out = []

    def conv(cin, cout, lvl, ldout, first=False, pool=False, head=False):
        cp = -(-cin // 4) * 4
        if first and cp == 4 and cin <= 3 and cout == 32:
            form, fused = "first_mfma", False
        elif first and cp == 4 and cin <= 4 and cout in (16, 32, 64):
            form, fused = "first_valu", False
        else:
            form, fused = _conv_form(cp, cout, hs[lvl], ws[lvl], ldout, 0, pool, head, sw)
        out.append((form + ("+pool" if fused else ""), cin, cout))
        if pool and not fused:
            out.append(("maxpool2", cout, cout))

    cin, c = cin0, f
    for i in range(depth):
        conv(cin, c, i, c, first=i == 0)
        conv(c, c, i, 2 * c, pool=True)
        cin, c = c, 2 * c
    conv(cin, c, depth, c)
    conv(c, c, depth, c)
    head_done = False
    for i in reversed(range(depth)):
        lo = f << i
        out.append(("convt_x3" if (2 * lo) % 32 == 0 and lo % 32 == 0 else "convt_generic", 2 * lo, lo))
        conv(2 * lo, lo, i, lo)
        conv(lo, lo, i, lo, head=head_wanted and i == 0)
        head_done = out[-1][0] == "wino_asm_cp1r2_head"
    q = f // 4
    if head_done:
        out.append(("patch_sum_combine", f, f))
    elif f % 4 == 0 and 1 <= ncls <= 4 and q <= 32 and q & (q - 1) == 0:          # patch_mean_head_fusable
        out.append(("patch_mean_head", f, ncls))
    else:
        out += [("head", f, ncls), ("patch_mean", f, f)]
    return out


def family_launches(cfg, shape, switches=None):
    """Profiling-record name -> launches of that forward."""
    out = {}
    for form, _, _ in layer_forms(cfg, shape, switches):
        name = RECORD[form.replace("+pool", "")]
        out[name] = out.get(name, 0) + 1
    return out


# ---- arithmetic tables ------------------------------------------------------------------------------------------------------------
class Ops(B.Ops):
    """bf16_oracle's table without a storage rounding, plus the passes after the last convolution."""

    @staticmethod
    def store(v):
        return v

    @staticmethod
    def head(f, w, b):
        return F.conv2d(f, w, b)

    @staticmethod
    def pmean(f):
        ph, pw = -f.shape[2] % PATCH, -f.shape[3] % PATCH
        return F.avg_pool2d(F.pad(f, (0, pw, 0, ph)), PATCH).permute(0, 2, 3, 1).reshape(-1, f.shape[1])    # the zero pad is in the divisor


EXACT = Ops("float64")


def _abs_conv3(x, w):
    return F.conv2d(x.abs(), w.abs(), padding=1)


ABS = Ops("float64 on absolute values", conv3=_abs_conv3, convt=lambda x, w, b: F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2),
          fold=lambda z, scale, shift: B.Ops.fold(z, scale.abs(), shift.abs()), pool=lambda x: F.max_pool2d(x.abs(), 2, 2))

_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def wino_conv3(x, w):
    """F(2x2,3x3) in x's dtype: U = G g G^T, V = B^T d B, M = sum_c U V, Y = A^T M A, every transform in that dtype."""
    dt = x.dtype
    G, BT, AT = (torch.tensor(m, dtype=dt) for m in (_G, _BT, _AT))
    Bn, C, H, W = x.shape
    th, tw = (H + 1) // 2, (W + 1) // 2
    xp = F.pad(x, (1, 2 * tw - W + 1, 1, 2 * th - H + 1))
    d = xp.unfold(2, 4, 2).unfold(3, 4, 2)                                # (B, C, th, tw, 4, 4)
    V = BT @ d @ BT.t()
    U = G @ w.to(dt) @ G.t()                                              # (N, C, 4, 4)
    M = torch.einsum("nckl,bcijkl->bnijkl", U, V)
    Y = AT @ M @ AT.t()                                                   # (B, N, th, tw, 2, 2)
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(Bn, w.shape[0], 2 * th, 2 * tw)[:, :, :H, :W].contiguous()


EMULATIONS = {"library_order_direct": Ops("library_order_direct", dtype=torch.float32),
              "winograd_f2x2_3x3": Ops("winograd_f2x2_3x3", dtype=torch.float32, conv3=wino_conv3)}


# ---- emulated broken kernels ------------------------------------------------------------------------------------------------------
def _as_fp32_path(ops):
    o = copy.copy(ops)
    o.store, o.head, o.pmean = Ops.store, Ops.head, Ops.pmean
    return o


def _pool_ceil(x):
    """Pooled rows laid out with the ceil-mode pitch on an odd level: the window grid of ceil mode read back with the floor geometry."""
    Bn, C, H, W = x.shape
    p = F.max_pool2d(x, 2, 2, ceil_mode=True)
    return p.reshape(Bn, C, -1)[:, :, :(H // 2) * (W // 2)].reshape(Bn, C, H // 2, W // 2)


class _PoolBeforeRelu(Ops):
    """The fused epilogue pools the folded value before its ReLU and stores that: a window of four negatives stays negative."""

    def __init__(self):
        super().__init__("pool_before_relu")
        self.pre = None

    def fold(self, z, scale, shift):
        self.pre = B.Ops.fold(z, scale, shift)
        return self.pre

    def pool(self, x):
        pre = self.pre if self.pre is not None and self.pre.shape == x.shape else x
        return F.max_pool2d(pre.to(x.dtype), 2, 2)


def _pmean_valid_divisor(f):
    ph, pw = -f.shape[2] % PATCH, -f.shape[3] % PATCH
    return F.avg_pool2d(F.pad(f, (0, pw, 0, ph)), PATCH, divisor_override=1).permute(0, 2, 3, 1).reshape(-1, f.shape[1]) / \
        F.avg_pool2d(F.pad(torch.ones_like(f[:, :1]), (0, pw, 0, ph)), PATCH, divisor_override=1).permute(0, 2, 3, 1).reshape(-1, 1)


MUTANTS = {n: _as_fp32_path(B.MUTANTS[n]) for n in ("bottom_halo_clamped", "stale_tap_buffer", "n_tail_dropped", "convt_quadrants_swapped",
                                                    "pad_row_written")}
MUTANTS.update({
    "pool_ceil_mode_odd_level": Ops("pool_ceil_mode_odd_level", pool=_pool_ceil),
    "pool_before_relu": _PoolBeforeRelu(),
    "head_reads_channel_c_plus_1": Ops("head_reads_channel_c_plus_1", head=lambda f, w, b: F.conv2d(f.roll(-1, dims=1), w, b)),
    "patch_mean_divides_by_valid_pixels": Ops("patch_mean_divides_by_valid_pixels", pmean=_pmean_valid_divisor),
})


# ---- the network, segment by segment ------------------------------------------------------------------------------------------------
def f64_params(p):
    return {k: (v.double() if v.dtype.is_floating_point else v) for k, v in p.items()}


def segment(p64, depth, name, src, ops=EXACT, eps=1e-5):
    """Exposed tensor `name` from its exposed predecessors in ops' arithmetic, float64 out (bf16_oracle.segment with Storage FP32)."""
    return B.segment(p64, depth, name, tuple(s.double() for s in src), False, ops, FP32, eps)[0]


def n_convs(depth, name):
    return 2 if name.startswith("skip") else 5 if name == f"feat{depth - 1}" else 3


def network(p64, x, depth, ops, eps=1e-5):
    """The forward in ops' arithmetic run through all segments on its own outputs: (logits, skips, feats, patch means), float64."""
    sk, ft = {}, {}
    if isinstance(ops, _PoolBeforeRelu):
        ops.pre = None
    for name in segment_names(depth):
        out = segment(p64, depth, name, sources(depth, name, x, sk, ft), ops, eps)
        (sk if name.startswith("skip") else ft)[int(name[4:])] = out
    f0 = ft[0]
    with torch.no_grad():
        lg = ops.head(f0, p64["decoder.final_conv.weight"], p64["decoder.final_conv.bias"])
        pm = ops.pmean(f0)
    return lg, [sk[i] for i in range(depth)], [ft[i] for i in range(depth)], pm


# ---- bar (a) ------------------------------------------------------------------------------------------------------------------------
def segment_bar(p64, depth, name, src):
    """(ref, S, c, {emulation: worst |emu - ref| / S}) of one segment on the sources `src`."""
    ref = segment(p64, depth, name, src)
    S = segment(p64, depth, name, src, ABS)
    ratios = {}
    for n, e in EMULATIONS.items():
        ratios[n] = float(((segment(p64, depth, name, src, e) - ref).abs() / S.clamp_min(1e-300)).max())
    return ref, S, max(C_FLOOR, C_FACTOR * max(ratios.values())), ratios


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar (an element whose bar is 0 must be equal), and the share of elements that differ at all."""
    err = (got.double() - ref).abs()
    r = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()), float((err > 0).double().mean())


def head_bar(f0, w64, b64):
    C = f0.shape[1]
    return C * 2.0 ** -24 * (F.conv2d(f0.double().abs(), w64.abs()) + b64.abs()[None, :, None, None])


def pmean_bar(f0):
    return 255 * 2.0 ** -24 * Ops.pmean(f0.double().abs())


def judge(p64, depth, x, got, tag="", show=print):
    """Bar (a) on one forward's outputs `got` = (logits, skips, feats, patch means), each tensor against the float64 reference computed
    from got's own predecessors.  Returns {tensor: (c, worst ratio to the bar, mismatch share)}; a ratio above 1 misses the bar."""
    lg, sk, ft, pm = got
    sk = [t.double() for t in sk]
    ft = [t.double() for t in ft]
    fig = {}
    for name in segment_names(depth):
        g = (sk if name.startswith("skip") else ft)[int(name[4:])]
        ref, S, c, ratios = segment_bar(p64, depth, name, sources(depth, name, x, sk, ft))
        worst, share = worst_ratio(g, ref, n_convs(depth, name) * c * S)
        fig[name] = (c, worst, share)
        show(f"    [{tag} {name}] L {n_convs(depth, name)}, c {c:.2e} (emulations: " + ", ".join(f"{n} {r:.2e}" for n, r in ratios.items()) +
             f"), worst |got - ref| / bar {worst:.3f}, mismatch {share * 100:.2f} %")
    w64, b64 = p64["decoder.final_conv.weight"], p64["decoder.final_conv.bias"]
    with torch.no_grad():
        worst, share = worst_ratio(lg, F.conv2d(ft[0], w64, b64), head_bar(ft[0], w64, b64))
        fig["logits"] = (ft[0].shape[1] * 2.0 ** -24, worst, share)
        wpm, spm = worst_ratio(pm, Ops.pmean(ft[0]), pmean_bar(ft[0]))
        fig["patch_means"] = (255 * 2.0 ** -24, wpm, spm)
    show(f"    [{tag}] logits <- feat0: worst / bar {worst:.3f}, mismatch {share * 100:.2f} %; patch means <- feat0: worst / bar {wpm:.3f}, "
         f"mismatch {spm * 100:.2f} %")
    return fig


def misses(fig):
    return [n for n, (_, worst, _) in fig.items() if not worst <= 1.0]


# ---- exact data (b) -----------------------------------------------------------------------------------------------------------------
EXACT_VAR = np.float32(1) - np.float32(1e-5)             # fl(var + 1e-5f) == 1.0f: bn_fold_kernel gives scale 1, shift 0
EXACT_EPS = 1.0 - float(EXACT_VAR)                       # the float64 network's eps with which var + eps == 1


def exact_params(cfg, seed):
    p = B.exact_params(cfg, seed)
    assert np.float32(EXACT_VAR + np.float32(1e-5)) == np.float32(1)
    for name in p:
        if name.endswith("running_var"):
            p[name] = torch.full_like(p[name], float(EXACT_VAR))
    return p


def exact_reference(p, x, depth):
    """The one right answer: (logits, skips, feats, patch means) of the float64 network with the BatchNorm scale exactly 1."""
    with torch.no_grad():
        lg, sk, ft = O.unet_forward(f64_params(p), x.double(), depth, eps=EXACT_EPS)
        return lg, sk, ft, Ops.pmean(ft[0])


def differing(got, ref):
    """Names of the tensors of a forward that are not bit for bit the reference's."""
    names = ["logits"] + [f"skip{i}" for i in range(len(ref[1]))] + [f"feat{i}" for i in range(len(ref[2]))] + ["patch_means"]
    flat = lambda o: [o[0]] + list(o[1]) + list(o[2]) + [o[3]]
    return [n for n, g, r in zip(names, flat(got), flat(ref)) if g.shape != r.shape or not torch.equal(g.double().cpu(), r)]
