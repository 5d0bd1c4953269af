"""Every kernel family that multiplies fp32 operands as three bf16 pieces (csrc/device.h), on operands built so that a lost piece
product shows: Winograd forward (C++ and assembly forms) and data gradient, ConvTranspose forward and data gradient, the Winograd
weight gradient <X3>, the first convolution and the GAT linear layer.

The suite's other bars (2e-5 or 1e-4 of the result's maximum) accept a kernel that drops a1 b1, a2 b0 or a0 b2
(tests/test_split_host.py pins that).  Here the error is measured against float64 in units of sum |a b| (split_oracle.err_units) and
barred by BAR[family, shape, case] of tests/test_split_host.py, which comes from the CPU alone: a quarter of the smallest error of
the emulated mutants the case is designated to catch, or, where a case designates none, four times the larger of the six-product
emulation's and the CPU fp32 run's error.  A correct kernel has about 4 x headroom over CPU fp32 (its summation order differs); every
designated mutant is at least 4 x over the bar.

Each call proves which kernel ran: by the profile record of the entry point where it writes one (mgu_conv2d_nhwc,
mgu_conv_transpose2x2_nhwc, mgu_unet_forward, the GAT layer), else by the bytes of the family's fp32 A/B arm, which must differ.
Output buffers are pre-filled with NaN.  Spatial sizes are small: this module tests arithmetic, tiling edges are covered elsewhere.

FAMILIES is the table both tiers read: the oracle's operation (split_oracle.FAMILY), the MGU_* switches of the context, what proves
the kernel, and the shapes.  DESIGNATED / EXCEPTIONS name, per operand case and family, the mutants the case must catch; the host tier
asserts the 16 x separation for each of them and that every mutant is designated in every family.

Measured on an MI355X with the kernels of commit b74c45a (this module's first run; no kernel missed a bar, none was changed): the
err_units of every (family, operand case), at the shape where it comes closest to its bar, beside that bar and the CPU fp32 run's
error.  Shapes are (B, H, W, Cin, Cout), (B, H, W, cin, layout) for the first convolution, (N, Fin, Fh, heads, concat) for the GAT.

family         case               worst shape              err_units       BAR   e_ref32
wino_fwd_cpp   normal             1-8-32-64-64              1.01e-07  1.79e-06  1.20e-07
wino_fwd_cpp   positive_low_bits  1-8-32-64-64              8.29e-07  8.91e-06  1.27e-06
wino_fwd_cpp   full_mantissa      1-8-32-64-64              1.21e-07  1.18e-06  1.20e-07
wino_fwd_cpp   cancellation       1-16-40-48-32             7.49e-08  5.89e-07  7.51e-08
wino_fwd_cpp   wide_exponents     1-8-32-64-64              8.54e-08  1.04e-06  1.35e-07
wino_fwd_cpp   bf16_exact         1-16-40-48-32             5.84e-08  3.41e-07  8.53e-08
wino_fwd_cpp   integers           1-8-32-64-64              0.00e+00  0.00e+00  0.00e+00
wino_fwd_asm   normal             1-8-32-64-64              1.01e-07  1.79e-06  1.20e-07
wino_fwd_asm   positive_low_bits  1-8-32-64-64              8.29e-07  8.91e-06  1.27e-06
wino_fwd_asm   full_mantissa      1-8-32-64-64              1.21e-07  1.18e-06  1.20e-07
wino_fwd_asm   cancellation       1-8-32-64-32              6.84e-08  4.73e-07  7.52e-08
wino_fwd_asm   wide_exponents     1-8-32-64-64              8.54e-08  1.04e-06  1.35e-07
wino_fwd_asm   bf16_exact         1-8-32-64-32              8.07e-08  3.14e-07  7.84e-08
wino_fwd_asm   integers           1-8-32-64-64              0.00e+00  0.00e+00  0.00e+00
wino_dgrad     normal             1-8-32-64-64              1.06e-07  1.88e-06  1.62e-07
wino_dgrad     positive_low_bits  1-8-32-64-64              8.17e-07  1.10e-05  1.17e-06
wino_dgrad     full_mantissa      1-8-32-32-32              1.20e-07  1.48e-06  1.56e-07
wino_dgrad     cancellation       1-8-32-64-64              7.84e-08  5.31e-07  6.81e-08
wino_dgrad     wide_exponents     1-8-32-64-64              1.01e-07  1.09e-06  1.10e-07
wino_dgrad     bf16_exact         1-8-32-32-32              6.16e-08  2.99e-07  7.48e-08
wino_dgrad     integers           1-8-32-64-64              0.00e+00  0.00e+00  0.00e+00
convt_fwd      normal             1-8-16-96-32              1.77e-07  2.81e-06  2.33e-07
convt_fwd      positive_low_bits  1-8-16-96-32              5.86e-07  4.94e-06  6.20e-07
convt_fwd      full_mantissa      1-8-16-96-32              1.91e-07  1.92e-06  1.90e-07
convt_fwd      cancellation       1-8-16-96-32              1.13e-07  8.42e-07  1.35e-07
convt_fwd      wide_exponents     1-8-16-96-32              1.96e-07  1.60e-06  2.16e-07
convt_fwd      bf16_exact         1-8-16-96-32              9.70e-08  3.88e-07  9.70e-08
convt_fwd      integers           1-8-16-32-32              0.00e+00  0.00e+00  0.00e+00
convt_dgrad    normal             1-8-16-64-32              2.10e-07  2.21e-06  2.05e-07
convt_dgrad    positive_low_bits  1-8-16-128-32             6.17e-07  4.68e-06  6.88e-07
convt_dgrad    full_mantissa      1-8-16-64-32              2.05e-07  1.61e-06  2.05e-07
convt_dgrad    cancellation       1-8-16-128-32             4.66e-08  1.20e-06  1.55e-07
convt_dgrad    wide_exponents     1-8-16-128-32             1.90e-07  1.29e-06  1.97e-07
convt_dgrad    bf16_exact         1-8-16-128-32             7.85e-08  4.57e-07  1.14e-07
convt_dgrad    integers           1-8-16-64-32              0.00e+00  0.00e+00  0.00e+00
wino_wgrad_x3  normal             1-8-16-64-64              1.75e-07  3.65e-06  1.76e-07
wino_wgrad_x3  positive_low_bits  1-8-16-64-64              4.81e-07  6.71e-06  5.57e-07
wino_wgrad_x3  full_mantissa      1-8-16-32-96              1.75e-07  2.55e-06  2.14e-07
wino_wgrad_x3  cancellation       1-8-16-64-64              8.07e-08  8.24e-07  9.73e-08
wino_wgrad_x3  bf16_exact         1-8-16-64-32              1.16e-07  4.48e-07  1.12e-07
wino_wgrad_x3  integers           1-8-16-64-64              0.00e+00  0.00e+00  0.00e+00
first_conv     normal             1-20-40-1-nchw            3.12e-07  6.94e-06  1.71e-07
first_conv     positive_low_bits  1-20-40-3-nchw            3.89e-07  5.38e-06  3.21e-07
first_conv     full_mantissa      1-20-40-2-nchw            2.73e-07  4.52e-06  1.92e-07
first_conv     cancellation       1-20-40-1-nchw            3.07e-07  5.18e-06  1.61e-07
first_conv     wide_exponents     1-20-40-2-nchw            3.01e-07  3.91e-06  2.00e-07
first_conv     bf16_exact         1-20-40-2-nchw            9.24e-08  3.33e-07  7.93e-08
first_conv     integers           1-20-40-1-nchw            0.00e+00  0.00e+00  0.00e+00
gat_linear     normal             200-64-64-4-1             1.70e-07  3.42e-06  2.26e-07
gat_linear     positive_low_bits  200-64-64-2-1             4.82e-07  4.14e-06  4.95e-07
gat_linear     full_mantissa      200-64-64-4-1             2.07e-07  2.35e-06  2.44e-07
gat_linear     cancellation       200-64-64-4-1             1.35e-07  1.13e-06  1.56e-07
gat_linear     wide_exponents     200-64-64-2-1             2.38e-07  2.10e-06  2.36e-07
gat_linear     bf16_exact         200-32-32-1-1             6.09e-08  2.43e-07  6.09e-08
gat_linear     integers           200-32-32-4-0             2.20e-08  8.80e-08  2.20e-08
gat_attention  positive_low_bits  200-32-64-4-1             3.65e-07  4.03e-06  4.69e-07
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import split_oracle as SO
from mgunet import _lib

pytestmark = pytest.mark.gpu

M = SO.ALL_MUTANTS
GROSS = ("drop_a0b0", "drop_a0b1", "drop_a1b0")
TWO_LOST = GROSS + ("two_pieces", "three_products")
# cancellation: both halves of b are equal, so the products of a0 with b's lower pieces cancel (a0 b2 exactly) with or without them
NOT_B2 = tuple(m for m in M if m not in ("drop_a0b2", "b2_zero", "drop_a0b1"))
# The mutants each operand case must catch, by kind of family, then the exceptions.  full_mantissa and wide_exponents isolate every
# product everywhere.  A mutant is designated only where the host emulation puts it at least 24 x above the CPU fp32 run, so that the
# asserted 16 x holds on another CPU's summation order too:
#   * normal data (signed lost terms average out) keeps the mutants that lose two products;
#   * Winograd forward / data gradient on all-positive operands: the transforms take differences of neighbours, so the lost terms do
#     not keep one sign, and the fp32 transforms themselves cost 1e-6 of sum |a b| there -- three products and worse stay clear;
#   * ConvTranspose on all-positive operands: fp32 accumulation of K = 96 .. 128 same-sign terms is itself at 7e-7, a1 b1 is 17 .. 22 x
#     above it (every other product 26 x and more); its data gradient under cancellation likewise keeps three products and worse.
DESIGNATED = {"normal": TWO_LOST, "positive_low_bits": M, "full_mantissa": M, "cancellation": NOT_B2, "wide_exponents": M, "bf16_exact": (),
              "integers": ()}
EXCEPTIONS = {
    ("wino_fwd_cpp", "positive_low_bits"): GROSS + ("three_products",), ("wino_fwd_asm", "positive_low_bits"): GROSS + ("three_products",),
    ("wino_dgrad", "positive_low_bits"): GROSS + ("three_products",), ("wino_wgrad_x3", "positive_low_bits"): TWO_LOST,
    ("convt_fwd", "positive_low_bits"): tuple(m for m in M if m != "drop_a1b1"),
    ("convt_dgrad", "positive_low_bits"): tuple(m for m in M if m != "drop_a1b1"),
    ("convt_dgrad", "cancellation"): ("drop_a0b0", "drop_a1b0", "three_products"),
}
# the weight gradient sums over pixels: exponents that change along a row meet inside one Winograd tile, where fp32 Winograd itself
# loses the small terms (1e-2 of sum |a b| in the host emulation) -- that case says nothing about the product and is left out there
FAMILIES = {
    "wino_fwd_cpp": dict(oracle="wino_fwd", env={"MGU_WINO_ASM": 0}, cases=SO.CASES,    # (B, H, W, Cin, Cout): proof label
                         shapes={(1, 8, 32, 64, 64): "wino3x3_cp_kernel<2>", (1, 16, 40, 32, 32): "wino3x3_cp_kernel<1>",
                                 (1, 16, 40, 48, 32): "wino3x3_cp_kernel<1>"}),
    "wino_fwd_asm": dict(oracle="wino_fwd", env={}, cases=SO.CASES,
                         shapes={(1, 8, 32, 64, 64): "mgu_wino_cp2_gfx950 (asm form of wino3x3_cp_kernel<2>)",
                                 (1, 8, 32, 32, 32): "mgu_wino_cp1r2_gfx950 (asm form of wino3x3_cp_kernel<1>)",
                                 (1, 8, 32, 64, 32): "mgu_wino_cp1r4_gfx950 (asm form of wino3x3_cp_kernel<1>)"}),
    "wino_dgrad": dict(oracle="wino_dgrad", env={}, ab={"MGU_WINO_PREC": 0}, cases=SO.CASES,
                       shapes={(1, 8, 32, 64, 64): None, (1, 8, 32, 32, 32): None}),
    "convt_fwd": dict(oracle="convt_fwd", env={}, cases=SO.CASES,
                      shapes={(1, 8, 16, 32, 32): "convt2x2_x3_kernel", (1, 8, 16, 64, 64): "convt2x2_x3_kernel",
                              (1, 8, 16, 96, 32): "convt2x2_x3_kernel"}),
    "convt_dgrad": dict(oracle="convt_dgrad", env={}, ab={"MGU_NO_CONVT_DGRAD_X3": 1}, cases=SO.CASES,
                        shapes={(1, 8, 16, 64, 32): None, (1, 8, 16, 128, 32): None}),
    "wino_wgrad_x3": dict(oracle="wino_wgrad", env={}, ab={"MGU_NO_WGRAD_X3": 1}, cases=tuple(c for c in SO.CASES if c != "wide_exponents"),
                          shapes={(1, 8, 16, 64, 64): None, (1, 8, 16, 64, 32): None, (1, 8, 16, 32, 96): None}),
    "first_conv": dict(oracle="first_conv", env={"MGU_NO_WINOGRAD": 1}, cases=SO.CASES,   # (B, H, W, cin, layout of x)
                       shapes={(1, 20, 40, ci, lay): "conv3x3_first_mfma_kernel" for ci in (1, 2, 3) for lay in ("nchw", "channels_last")}),
    "gat_linear": dict(oracle="gat_linear", env={}, cases=SO.CASES,                        # (N, Fin, Fh, heads, concat)
                       shapes={(200, 32, 32, 1, 1): "gat_fused2_kernel", (200, 32, 64, 2, 0): "gat_fused2_kernel",
                               (200, 64, 64, 4, 1): "gat_fused2_kernel", (200, 32, 32, 4, 0): "gat_fused2_kernel",
                               (200, 64, 64, 2, 1): "gat_fused2_kernel"}),
    # one more case of the GAT family: the softmax in (three in-neighbours, nonzero attention vectors), so that the aggregate the split
    # sees is the kernel's own; barred by the same rule with the oracle's float32 layer as the CPU fp32 run
    "gat_attention": dict(oracle="gat_attention", env={}, cases=("positive_low_bits",), extra=True,
                          shapes={(200, 32, 64, 4, 1): "gat_fused2_kernel"}),
}


def designated(family, case):
    return EXCEPTIONS.get((family, case), DESIGNATED[case])


def params(family):
    f = FAMILIES[family]
    return [pytest.param(shape, case, id="-".join(map(str, shape)) + "-" + case) for shape in f["shapes"] for case in f["cases"]]


# ---- contexts and proofs ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def environment(**env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def context(cuda, **env):
    """A fresh mgu_ctx created under the given MGU_* switches (they are read at mgu_create and live in the context)."""
    with environment(**env):
        ctx = _lib.Context(cuda.index or 0)
    yield ctx
    torch.cuda.synchronize()


@contextlib.contextmanager
def recorded(ctx, names):
    """Profile records of the calls made inside: their kernel labels are appended to `names`."""
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    yield
    torch.cuda.synchronize()
    names.extend(k["name"] for k in _lib.read_kernel_stats(ctx))
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)


def nhwc(a):
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1)))


def nchw(t):
    return np.ascontiguousarray(t.permute(0, 3, 1, 2).cpu().numpy())


def nan(cuda, *shape):
    return torch.full(shape, float("nan"), device=cuda)


# ---- one GPU run per family: (ctx, shape, a, b) -> the result in the layout of the oracle's family ----------------------------------
def run_wino_fwd(cuda, ctx, shape, a, b):
    B, H, W, Ci, Co = shape
    xin, wd, out = nhwc(a).to(cuda), torch.from_numpy(b).to(cuda), nan(cuda, B, H, W, Co)
    _lib.check(_lib.lib().mgu_conv2d_nhwc(ctx.handle, xin.data_ptr(), B, H, W, Ci, wd.data_ptr(), None, None, None, Co, 3, 0, out.data_ptr(),
                                          Co, 0, _lib.current_stream_ptr(cuda)), ctx.handle)
    return nchw(out)


def run_wino_dgrad(cuda, ctx, shape, a, b):
    B, H, W, Ci, Co = shape
    dz, wd, din = nhwc(a).to(cuda), torch.from_numpy(b).to(cuda), nan(cuda, B, H, W, Ci)
    _lib.check(_lib.lib().mgu_conv2d_dgrad_nhwc(ctx.handle, dz.data_ptr(), wd.data_ptr(), B, H, W, Ci, Co, 3, din.data_ptr(), Ci,
                                                _lib.current_stream_ptr(cuda)), ctx.handle)
    return nchw(din)


def run_wino_wgrad(cuda, ctx, shape, a, b):
    B, H, W, Ci, Co = shape
    xin, dz, dw = nhwc(a).to(cuda), nhwc(b).to(cuda), nan(cuda, Co, Ci, 3, 3)
    _lib.check(_lib.lib().mgu_conv2d_wgrad_nhwc(ctx.handle, xin.data_ptr(), Ci, dz.data_ptr(), B, H, W, Ci, Co, 3, dw.data_ptr(),
                                                _lib.current_stream_ptr(cuda)), ctx.handle)
    return dw.cpu().numpy()


def run_convt_fwd(cuda, ctx, shape, a, b):
    """Into the upper channel half of a 2 Cout buffer, as the U-Net's concat buffers receive it; the lower half stays untouched."""
    B, H, W, Ci, Co = shape
    xin, wd, bias, out = nhwc(a).to(cuda), torch.from_numpy(b).to(cuda), torch.zeros(Co, device=cuda), nan(cuda, B, 2 * H, 2 * W, 2 * Co)
    _lib.check(_lib.lib().mgu_conv_transpose2x2_nhwc(ctx.handle, xin.data_ptr(), B, H, W, Ci, wd.data_ptr(), bias.data_ptr(), Co, out.data_ptr(),
                                                     2 * Co, Co, _lib.current_stream_ptr(cuda)), ctx.handle)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[..., :Co]).all())
    return nchw(out[..., Co:])


def run_convt_dgrad(cuda, ctx, shape, a, b):
    """The gradient arrives in the upper channel half of a concat-shaped buffer; the lower half is NaN and must not be read."""
    B, H, W, Ci, Co = shape
    dcat = nan(cuda, B, 2 * H, 2 * W, 2 * Co)
    dcat[..., Co:] = nhwc(a).to(cuda)
    wd, din = torch.from_numpy(b).to(cuda), nan(cuda, B, H, W, Ci)
    _lib.check(_lib.lib().mgu_conv_transpose2x2_dgrad_nhwc(ctx.handle, dcat.data_ptr(), 2 * Co, Co, wd.data_ptr(), B, H, W, Ci, Co, din.data_ptr(),
                                                           _lib.current_stream_ptr(cuda)), ctx.handle)
    return nchw(din)


def identity_variance():
    """A float32 running variance v with fl(v + 1e-5f) == 1, so that the eval fold gamma / sqrtf(v + eps) of gamma = 1 is exactly 1."""
    eps, v = np.float32(1e-5), np.float32(1) - np.float32(1e-5)
    for _ in range(4):
        if np.float32(v + eps) == np.float32(1):
            return float(v)
        v = np.nextafter(v, np.float32(2) if np.float32(v + eps) < 1 else np.float32(0), dtype=np.float32)
    raise AssertionError("no float32 variance folds to scale 1")


def run_first_conv(cuda, ctx_env, shape, a, b, names):
    """mgu_conv2d_nhwc rejects Cin = 3: the kernel is reached through UNet(cin, 2, 32, 1) in eval mode.  Both BatchNorms of the first
    block fold to scale 1 / shift 0 and its second convolution is the centre-tap identity with zero bias, so the level-0 skip is
    relu(conv1(x)) passed through exact x * 1 + 0 sums (MGU_NO_WINOGRAD=1: the fp32 direct kernel, no transform roundings)."""
    import mgunet
    import mgunet_oracle as O
    B, H, W, ci, layout = shape
    p = O.make_unet_params(ci, 2, 32, 1, seed=ci)
    blk = "encoder.encoder_blocks.0."
    ident = torch.zeros(32, 32, 3, 3)
    ident[torch.arange(32), torch.arange(32), 1, 1] = 1.0
    p[blk + "conv1.weight"], p[blk + "conv2.weight"] = torch.from_numpy(b).clone(), ident
    for n in ("1", "2"):
        p[blk + f"conv{n}.bias"], p[blk + f"bn{n}.bias"], p[blk + f"bn{n}.running_mean"] = torch.zeros(32), torch.zeros(32), torch.zeros(32)
        p[blk + f"bn{n}.weight"], p[blk + f"bn{n}.running_var"] = torch.ones(32), torch.full((32,), identity_variance())
    model = mgunet.UNet(ci, 2, 32, 1)
    model.load_state_dict(p)
    model = model.to(cuda).eval()
    with environment(**ctx_env):
        ctx = model._context(cuda)
    model._sync_weights(ctx, cuda)
    x = torch.from_numpy(a).to(cuda)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    logits, cat, feat = nan(cuda, B, H, W, 2), nan(cuda, B, H, W, 64), nan(cuda, B, H, W, 32)
    with recorded(ctx, names):
        _lib.call("mgu_unet_forward", cuda, x, B, H, W, *x.stride(), logits, (C.c_void_p * 1)(cat.data_ptr()), (C.c_void_p * 1)(feat.data_ptr()),
                  0, ctx=ctx)
    assert bool(torch.isfinite(logits).all()) and bool(torch.isfinite(cat).all()) and bool(torch.isfinite(feat).all())
    return nchw(cat[..., :32])


def ring_csr(cuda, N):
    """CSR by target of the graph in which node i has the single in-neighbour (i + 7) % N."""
    rowptr = torch.arange(N + 1, dtype=torch.int32)
    col = torch.from_numpy(SO.GatLinear.src(N).astype(np.int32))
    return rowptr.to(cuda), col.to(cuda)


def run_gat_linear(cuda, ctx, shape, a, b):
    N, Fin, Fh, heads, concat = shape
    rowptr, col = ring_csr(cuda, N)
    X, Wd, att = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda), torch.zeros(heads, 2 * Fh, device=cuda)
    out = nan(cuda, N, heads * Fh if concat else Fh)
    _lib.check(_lib.lib().mgu_gat_layer_forward(ctx.handle, X.data_ptr(), N, Fin, rowptr.data_ptr(), col.data_ptr(), N, None, 1, Wd.data_ptr(),
                                                att.data_ptr(), heads, Fh, concat, 0.2, out.data_ptr(), _lib.current_stream_ptr(cuda)),
               ctx.handle)
    return out.cpu().numpy()


def run_gat_attention(cuda, ctx, shape, a, b):
    N, Fin, Fh, heads, concat = shape
    fam = SO.FAMILY["gat_attention"]
    src, tgt = fam.edges(N)
    deg = len(fam.SHIFTS)
    rowptr, col = (deg * torch.arange(N + 1, dtype=torch.int32)).to(cuda), torch.from_numpy(src.astype(np.int32)).to(cuda)
    X, Wd, att = torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda), torch.from_numpy(fam.att(shape)).to(cuda)
    out = nan(cuda, N, heads * Fh if concat else Fh)
    _lib.check(_lib.lib().mgu_gat_layer_forward(ctx.handle, X.data_ptr(), N, Fin, rowptr.data_ptr(), col.data_ptr(), deg * N, None, 1,
                                                Wd.data_ptr(), att.data_ptr(), heads, Fh, concat, 0.2, out.data_ptr(),
                                                _lib.current_stream_ptr(cuda)), ctx.handle)
    return out.cpu().numpy()


RUN = {"gat_attention": run_gat_attention, "wino_fwd": run_wino_fwd, "wino_dgrad": run_wino_dgrad, "wino_wgrad": run_wino_wgrad, "convt_fwd": run_convt_fwd,
       "convt_dgrad": run_convt_dgrad, "gat_linear": run_gat_linear}


def gpu_result(cuda, family, shape, case, a, b):
    """The family's kernel on (a, b), with the proof that it was that kernel: the profile label where the table names one, else
    different bytes from the fp32 A/B arm."""
    f = FAMILIES[family]
    label, names = f["shapes"][shape], []
    if f["oracle"] == "first_conv":
        got = run_first_conv(cuda, f["env"], shape, a, b, names)
    else:
        with context(cuda, **f["env"]) as ctx:
            if label:
                with recorded(ctx, names):
                    got = RUN[f["oracle"]](cuda, ctx, shape, a, b)
            else:
                got = RUN[f["oracle"]](cuda, ctx, shape, a, b)
    if label:
        assert label in names, (label, names)
    else:
        if case == "integers":   # both arms are exact there: the proof runs on the family's normal operands
            a, b = SO.FAMILY[f["oracle"]].make(shape, "normal")
            with context(cuda, **f["env"]) as ctx:
                mine = RUN[f["oracle"]](cuda, ctx, shape, a, b)
        else:
            mine = got
        with context(cuda, **dict(f["env"], **f["ab"])) as ctx:
            other = RUN[f["oracle"]](cuda, ctx, shape, a, b)
        assert np.isfinite(other).all() and not np.array_equal(mine, other), "the A/B arm gave the same bytes: which kernel ran?"
    return got


def check(cuda, family, shape, case, record=None):
    from test_split_host import BAR, reference
    fam = SO.FAMILY[FAMILIES[family]["oracle"]]
    a, b = fam.make(shape, case)
    got = gpu_result(cuda, family, shape, case, a, b)
    ref, scale = reference(FAMILIES[family]["oracle"], shape, case)
    e, bar = SO.err_units(got, ref, scale), BAR[family, shape, case]
    print(f"MEASURED {family} {'-'.join(map(str, shape))} {case}: err_units {e:.2e} bar {bar:.2e}")
    assert not np.isnan(got).any()
    if case == "integers":
        exact = np.ones(ref.shape, bool)
        if family == "gat_linear":      # ELU of a negative sum is not an integer: bit equality where every head's sum is >= 0
            N, Fin, Fh, heads, concat = shape
            pre = fam.direct(shape, a.astype(np.float64), b.astype(np.float64)) >= 0
            exact = pre if concat else pre.reshape(N, heads, Fh).all(1)
        assert exact.any() and np.array_equal(got.astype(np.float64)[exact], ref[exact])
    assert SO.passes(got, ref, scale, bar), (e, bar)
    return got


@pytest.mark.parametrize("shape,case", params("wino_fwd_cpp"))
def test_winograd_forward_cpp(cuda, shape, case):
    """wino3x3_cp_kernel<2> (64 output channels per workgroup) and <1> (32, with an even and an odd chunk count)."""
    check(cuda, "wino_fwd_cpp", shape, case)


@pytest.mark.parametrize("shape,case", params("wino_fwd_asm"))
def test_winograd_forward_asm(cuda, shape, case):
    """The assembly forms, and on these operands too the bytes of the C++ kernel they replace."""
    got = check(cuda, "wino_fwd_asm", shape, case)
    a, b = SO.FAMILY["wino_fwd"].make(shape, case)
    names = []
    with context(cuda, MGU_WINO_ASM=0) as ctx, recorded(ctx, names):
        cpp = run_wino_fwd(cuda, ctx, shape, a, b)
    assert names and names[0].startswith("wino3x3_cp_kernel"), names
    assert np.array_equal(got, cpp)


@pytest.mark.parametrize("shape,case", params("wino_dgrad"))
def test_winograd_data_gradient(cuda, shape, case):
    check(cuda, "wino_dgrad", shape, case)


@pytest.mark.parametrize("shape,case", params("convt_fwd"))
def test_conv_transpose_forward(cuda, shape, case):
    check(cuda, "convt_fwd", shape, case)


@pytest.mark.parametrize("shape,case", params("convt_dgrad"))
def test_conv_transpose_data_gradient(cuda, shape, case):
    check(cuda, "convt_dgrad", shape, case)


@pytest.mark.parametrize("shape,case", params("wino_wgrad_x3"))
def test_winograd_weight_gradient_x3(cuda, shape, case):
    check(cuda, "wino_wgrad_x3", shape, case)


@pytest.mark.parametrize("shape,case", params("first_conv"))
def test_first_convolution(cuda, shape, case):
    check(cuda, "first_conv", shape, case)


@pytest.mark.parametrize("shape,case", params("gat_linear"))
def test_gat_linear_layer(cuda, shape, case):
    check(cuda, "gat_linear", shape, case)


@pytest.mark.parametrize("shape,case", params("gat_attention"))
def test_gat_layer_with_attention(cuda, shape, case):
    check(cuda, "gat_attention", shape, case)
