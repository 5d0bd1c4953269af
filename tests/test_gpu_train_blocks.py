"""The train-mode half block -- Conv2d(3x3) -> BatchNorm2d(batch statistics) -> ReLU [-> MaxPool2d(2)] -- and its backward, each
in isolation against FLOAT64 torch on the CPU, through the functions the training step itself runs per layer (include/mgunet.h
"train-step building blocks": conv_bn_relu_train / conv_bn_relu_backward of mgunet_train.hip on a FwdRecord of the caller's tensors).  What the
whole-step tests (test_gpu_train.py) see only through 1e-3 logits and a gradient whose conditioning hides a 1 % kernel error is
held here to the kernels' own bar, 2e-5 of the result's max: the statistics the six Winograd kernel forms accumulate in their
epilogue, their fold (bn_finalize_slots_kernel), the pooled apply pass, the deferred bias-gradient fold of the gradient unpack
launch, and the zero-between-launches invariant of the reduction slots all of them share.

Replaces, per layer, model/unet/unet_encoder.py:15-25,48 and its autograd nodes (scripts/train_segmentation.py:121-133)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mgunet_oracle as O
from mgunet import _lib
from test_gpu_backward_kernels import TOL, context, nhwc, rel

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
SENTINEL = -7.0          # y is >= 0: a channel of the ld_y buffer outside [0, C) must keep this value
# max over layers and channels of |mean| / std of z in the float64 oracle forward (train mode) of config (3, 2, 32, 4) on the c5
# inputs: 4.60 / 5.06 (2 x 128^2 / 4 x 512^2 shard) with the golden step's initial parameters, 4.53 / 5.14 after its Adam step
# (NOTES.md "Train-forward block"; recomputed by tests/test_train_blocks_host.py).  The offset-channel inputs below reach twice that: drift over a training run is unmeasured.
R_OBS = 5.14

FWD_ENVS = {"default": {}, "no_wino_cp": {"MGU_NO_WINO_CP": 1}, "fp32_mfma": {"MGU_WINO_PREC": 0}, "no_winograd": {"MGU_NO_WINOGRAD": 1}}
# the Winograd kernel form a variant must run (wide: Cout > 32), as the profile read-out names it
WINO_NAME = {"default": ("wino3x3_cp_kernel<2>", "wino3x3_cp_kernel<1>"), "no_wino_cp": ("wino3x3_f32_kernel<0,1>", "wino3x3_f32_kernel<1,1>"),
             "fp32_mfma": ("wino3x3_f32_kernel<0,0>", "wino3x3_f32_kernel<1,0>")}

FWD_CASES = {  # B, H, W, Cin, Cout
    "one_partial_patch": (1, 5, 7, 16, 32),        # less than one 8 x 32 patch, M = 35
    "wide_even": (2, 12, 10, 64, 64),              # wide split; even sizes: the apply pass also pools
    "ragged_odd": (1, 9, 70, 32, 96),              # ragged patches, odd H: the pool kernel runs on y
    "n_tail": (3, 16, 32, 48, 40),                 # N = 40 of a 64-channel workgroup: the epilogue's n < d.N guards
    "three_n_blocks": (1, 31, 33, 128, 160),
    # wino_plan: 3 x 3 patches per image x 57 images = 513 patches, one n block -> ppb = 513 / 256 = 2 patches per workgroup (257 patch
    # groups, 264 workgroups <= STAT_ROWS) on the narrow kernel (Cout 32) and on the wide one (Cout 48): per-thread sums run across patches
    "two_patches_narrow": (57, 17, 65, 32, 32),
    "two_patches_wide": (57, 17, 65, 32, 48),
    "direct_cin8": (2, 13, 17, 8, 32),             # Cin % 16 != 0: no Winograd kernel, statistics by their own pass
    "first_conv": (2, 16, 16, 3, 32),              # Cin 3 on the packed 4-channel input: the first-conv kernels
}


def bn_params(name, C):
    gamma = torch.from_numpy(O.formula_uniform(name + "/gamma", (C,), 0.5, 1.5, seed=C))
    gamma[1::5] *= -1
    beta = torch.from_numpy(O.formula_uniform(name + "/beta", (C,), -0.5, 0.5, seed=C))
    rm = torch.from_numpy(O.formula_uniform(name + "/rm", (C,), -0.2, 0.2, seed=C))
    rv = torch.from_numpy(O.formula_uniform(name + "/rv", (C,), 0.5, 1.5, seed=C))
    return gamma, beta, rm, rv


def forward_reference(x, w, b, gamma, beta, rm, rv):
    """float64 torch on the CPU: conv2d -> batch_norm(training) -> relu; computed once per input and never modified."""
    z = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    rmd, rvd = rm.double().clone(), rv.double().clone()
    y = F.relu(F.batch_norm(z, rmd, rvd, gamma.double(), beta.double(), training=True, momentum=MOM, eps=EPS))
    mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
    return {"z": z, "y": y, "mean": mean, "var": var, "invstd": 1.0 / torch.sqrt(var + EPS), "run_mean": rmd, "run_var": rvd}


@functools.lru_cache(maxsize=None)
def plain_case(name):
    B, H, W, Cin, Cout = FWD_CASES[name]
    x = torch.from_numpy(O.formula_normal("tb/x", (B, Cin, H, W), seed=Cin + H))
    a = 0.9 * float(np.sqrt(6.0 / (9 * Cin)))
    w = torch.from_numpy(O.formula_uniform("tb/w", (Cout, Cin, 3, 3), -a, a, seed=Cout))
    b = torch.from_numpy(O.formula_uniform("tb/b", (Cout,), -0.1, 0.1, seed=Cout))
    inp = (x, w, b) + bn_params("tb", Cout)
    return inp, forward_reference(*inp)


def run_forward(cuda, ctx, inp, pad_y=8, pool=True):
    """mgu_conv_bn_relu_train_nhwc on fresh output buffers; returns them (on the device) with the two path reports and the name of
    the convolution kernel."""
    x, w, b, gamma, beta, rm, rv = inp
    B, Cin, H, W = x.shape
    Cout, Cp, ld_y = w.shape[0], (Cin + 3) // 4 * 4, w.shape[0] + pad_y
    xin = torch.zeros((B, H, W, Cp), device=cuda)
    xin[..., :Cin] = nhwc(x).to(cuda)
    dev = [t.contiguous().to(cuda) for t in (w, b, gamma, beta)]
    o = {"z": torch.full((B, H, W, Cout), float("nan"), device=cuda), "ybuf": torch.full((B, H, W, ld_y), SENTINEL, device=cuda),
         "pooled": torch.full((B, H // 2, W // 2, Cout), float("nan"), device=cuda) if pool else None,
         "mean": torch.full((Cout,), float("nan"), device=cuda), "invstd": torch.full((Cout,), float("nan"), device=cuda),
         "run_mean": rm.clone().to(cuda), "run_var": rv.clone().to(cuda)}
    sf, pf = C.c_int(-1), C.c_int(-1)
    L = _lib.lib()
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    _lib.check(L.mgu_conv_bn_relu_train_nhwc(ctx.handle, xin.data_ptr(), Cp, B, H, W, Cin, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                             dev[3].data_ptr(), Cout, o["z"].data_ptr(), o["ybuf"].data_ptr(), ld_y,
                                             o["pooled"].data_ptr() if pool else None, o["mean"].data_ptr(), o["invstd"].data_ptr(),
                                             o["run_mean"].data_ptr(), o["run_var"].data_ptr(), C.byref(sf), C.byref(pf),
                                             _lib.current_stream_ptr(cuda)), ctx.handle)
    torch.cuda.synchronize()
    o["kernels"] = [k["name"] for k in _lib.read_kernel_stats(ctx)]
    _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    o["stats_fused"], o["pool_fused"] = sf.value, pf.value
    o["y"] = o["ybuf"][..., :Cout]
    return o


def forward_errors(o, ref):
    e = {k: rel(o[k].permute(0, 3, 1, 2), ref[k]) for k in ("z", "y")}
    e.update({k: rel(o[k], ref[k]) for k in ("mean", "run_mean", "run_var")})
    e["invstd"] = float(((o["invstd"].double().cpu() - ref["invstd"]).abs() / ref["invstd"]).max())   # relative, per channel
    return e


def check_forward(o, ref, tag):
    e = forward_errors(o, ref)
    print(f"[train-block {tag}] stats_fused {o['stats_fused']} pool_fused {o['pool_fused']} {o['kernels']} " +
          " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    Cout = o["z"].shape[-1]
    if o["pooled"] is not None:   # MaxPool2d(2) of the GPU's own y, bit for bit
        assert torch.equal(o["pooled"].permute(0, 3, 1, 2), F.max_pool2d(o["y"].permute(0, 3, 1, 2), 2))
    assert bool((o["ybuf"][..., Cout:] == SENTINEL).all())
    assert all(v <= TOL for v in e.values()), e   # (every entry: a NaN fails its own comparison)
    return e


# ---- (a) forward, per kernel form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(FWD_ENVS))
@pytest.mark.parametrize("case", list(FWD_CASES))
def test_forward_block_vs_float64(cuda, variant, case):
    B, H, W, Cin, Cout = FWD_CASES[case]
    inp, ref = plain_case(case)
    with context(cuda, **FWD_ENVS[variant]) as ctx:
        o = run_forward(cuda, ctx, inp)
        wino = Cin % 16 == 0 and variant != "no_winograd"
        assert o["stats_fused"] == int(wino) and o["pool_fused"] == int(H % 2 == 0 and W % 2 == 0)
        if wino:
            assert WINO_NAME[variant][0 if Cout > 32 else 1] in o["kernels"], o["kernels"]
        check_forward(o, ref, f"{case}/{variant}")


# ---- (b) a grid larger than the statistics table ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_grid_case():
    # 8 x 20 patches x 4 images = 640 one-patch workgroups under MGU_WINO_PPB_CAP=1: more than STAT_ROWS = 576 table rows, so the
    # statistics take their own pass; uncapped the plan walks 2 patches per workgroup (320 groups) and the epilogue accumulates them
    B, H, W, Cin, Cout = 4, 160, 256, 16, 32
    x = torch.from_numpy(O.formula_normal("tb/x", (B, Cin, H, W), seed=Cin + H))
    a = 0.9 * float(np.sqrt(6.0 / (9 * Cin)))
    w = torch.from_numpy(O.formula_uniform("tb/w", (Cout, Cin, 3, 3), -a, a, seed=Cout))
    b = torch.from_numpy(O.formula_uniform("tb/b", (Cout,), -0.1, 0.1, seed=Cout))
    inp = (x, w, b) + bn_params("tb", Cout)
    return inp, forward_reference(*inp)


@pytest.mark.parametrize("cap,fused", [(1, 0), (None, 1)])
def test_forward_block_grid_beyond_stat_rows(cuda, cap, fused):
    inp, ref = big_grid_case()
    with context(cuda, **({"MGU_WINO_PPB_CAP": cap} if cap else {})) as ctx:
        o = run_forward(cuda, ctx, inp)
        assert o["stats_fused"] == fused and o["pool_fused"] == 1
        assert "wino3x3_cp_kernel<1>" in o["kernels"], o["kernels"]
        check_forward(o, ref, f"big_grid/cap={cap}")


# ---- (d) offset channels, (e) degenerate channels --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def offset_case(name):
    """Channels whose |mean| / std of z spreads from 0 to 2 * R_OBS: non-negative activations, weights with a per-channel offset on
    every other channel, and a bias that tops each channel up to its target ratio (so the offset comes from the weights AND the bias)."""
    B, H, W, Cin, Cout = FWD_CASES[name]
    x = torch.from_numpy(O.formula_normal("tb/off/x", (B, Cin, H, W), seed=Cin + H)).abs()
    a = 0.9 * float(np.sqrt(6.0 / (9 * Cin)))
    w = torch.from_numpy(O.formula_uniform("tb/off/w", (Cout, Cin, 3, 3), -a, a, seed=Cout))
    w[1::2] += 0.5 * a * torch.linspace(0, 1, Cout)[1::2].view(-1, 1, 1, 1)
    z0 = F.conv2d(x.double(), w.double(), padding=1)
    m0, s0 = z0.mean((0, 2, 3)), z0.std((0, 2, 3), unbiased=False)
    target = torch.linspace(0, 2.04 * R_OBS, Cout, dtype=torch.float64)
    sign = torch.where(torch.arange(Cout) % 4 < 2, 1.0, -1.0).double()
    b = (sign * target * s0 - m0).float()
    inp = (x, w, b) + bn_params("tb/off", Cout)
    return inp, forward_reference(*inp)


def offset_ratio(ref):
    return ref["mean"].abs() / torch.sqrt(ref["var"])


OFFSET_RUNS = [("wide_even", "default"), ("two_patches_narrow", "default"), ("two_patches_wide", "default"), ("two_patches_wide", "no_wino_cp"),
               ("two_patches_wide", "fp32_mfma"), ("wide_even", "no_winograd"), ("two_patches_wide", "no_winograd")]


@pytest.mark.parametrize("case,variant", OFFSET_RUNS)
def test_forward_block_offset_channels(cuda, case, variant):
    """var = sum z^2 / M - (sum z / M)^2 from fp32 per-thread partial sums loses (|mean| / std)^2 * 1e-7 of the variance.  At twice the
    ratio the network shows, the bars hold as the code stands: worst invstd 8.6e-7 (epilogue) / 7.0e-7 (own pass), run_var 1.0e-6, y
    8.8e-7 / 2.0e-6 of the maximum, where torch's own fp32 forward is 7.3e-7 to 1.0e-6 from float64 on the same inputs."""
    inp, ref = offset_case(case)
    r = offset_ratio(ref)
    # the spread the inputs were built for, verified on the float64 reference: from 0 up to twice the observed ratio, no large gap
    assert float(r.min()) <= 0.05 and float(r.max()) >= 2 * R_OBS, (float(r.min()), float(r.max()))
    assert float(r.sort().values.diff().max()) <= 0.1 * 2 * R_OBS
    with context(cuda, **FWD_ENVS[variant]) as ctx:
        o = run_forward(cuda, ctx, inp)
        assert o["stats_fused"] == int(variant != "no_winograd")
        x = inp[0]
        with torch.no_grad():   # torch's own fp32 forward on the CPU against float64, for context (NOTES.md)
            z32 = F.conv2d(x, inp[1], inp[2], padding=1)
            y32 = F.relu(F.batch_norm(z32, inp[5].clone(), inp[6].clone(), inp[3], inp[4], training=True, momentum=MOM, eps=EPS))
        print(f"[train-block offset {case}/{variant}] max |mean|/std {float(r.max()):.2f} max |mean| {float(ref['mean'].abs().max()):.2f}; "
              f"torch fp32 vs float64: z {rel(z32, ref['z']):.2e} y {rel(y32, ref['y']):.2e}")
        check_forward(o, ref, f"offset/{case}/{variant}")


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """The offset inputs of the wide_even shape with a constant channel (zero weights, bias = the largest channel mean of the offset
    inputs), a negative gamma and a zero gamma."""
    (x, w, b, gamma, beta, rm, rv), ref0 = offset_case("wide_even")
    w, b, gamma = w.clone(), b.clone(), gamma.clone()
    w[0] = 0.0
    b[0] = float(ref0["mean"].abs().max())
    gamma[1] = -abs(float(gamma[1])) - 0.5
    gamma[2] = 0.0
    inp = (x, w, b, gamma, beta, rm, torch.ones_like(rv))
    return inp, forward_reference(*inp)


@pytest.mark.parametrize("variant", ["default", "no_wino_cp", "fp32_mfma", "no_winograd"])
def test_forward_block_degenerate_channels(cuda, variant):
    """A constant channel's true variance is 0; the computed one is rounding noise next to eps = 1e-5.  Measured as the code stands,
    with b = 40.0: variance 5.1e-5 from the epilogue's sums (run_var 5.1e-6 from 0.9), 2.4e-7 from the separate pass; the channel's y
    is 1.8e-5 / 1.4e-5 of the tensor's maximum from relu(beta) -- inside the bar by a tenth.  That error is not the variance's: it is
    the rounding of shift = beta - mean * scale and of z * scale + shift at |mean * scale| = 40 * gamma / sqrt(var + eps) = 3800 to 9400,
    whose ulp is 2.4e-4 to 9.8e-4.  An fp32 emulation of the apply pass gives 8e-6 to 2.9e-4 of the maximum over var in {5.1e-5, 2.4e-7,
    0} and the last bit of the mean: this input sits at the low end, and an exactly zero variance alone would not improve it
    (NOTES.md "Train-forward block").  The results are bitwise reproducible, so the figure does not move from run to run."""
    inp, ref = degenerate_case()
    beta = inp[4]
    assert float(ref["var"][0]) == 0.0 and float((ref["y"][:, 0] - F.relu(beta[0].double())).abs().max()) <= 1e-12
    with context(cuda, **FWD_ENVS[variant]) as ctx:
        o = run_forward(cuda, ctx, inp)
        assert o["stats_fused"] == int(variant != "no_winograd")
        e = {"y": rel(o["y"].permute(0, 3, 1, 2), ref["y"]), "mean": rel(o["mean"], ref["mean"]),
             "y_const": float((o["y"][..., 0].double().cpu() - F.relu(beta[0].double())).abs().max()) / float(ref["y"].abs().max()),
             "run_var_const": abs(float(o["run_var"][0]) - 0.9)}
        print(f"[train-block degenerate/{variant}] b {float(inp[2][0]):.3f} " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert e["y"] <= TOL and e["mean"] <= TOL and e["run_var_const"] <= 2e-5, e


# ---- (f) backward half block ------------------------------------------------------------------------------------------------------
BWD_CASES = [(2, 13, 17, 8, 32), (2, 24, 40, 32, 32), (2, 35, 18, 96, 64), (1, 16, 16, 256, 128), (2, 37, 45, 64, 64)]
BWD_ENVS = {"default": {}, "no_wino_wgrad": {"MGU_NO_WINO_WGRAD": 1}, "no_wino_dgrad": {"MGU_NO_WINO_DGRAD": 1}}
MASK_EXACT = 1e-6    # a ReLU mask may differ from float64's only where |pre-ReLU y| is below this
DZ_SKIP = 1e-5       # elements this close to the kink may be left out of the dz comparison (at most DZ_SKIP_CAP of them)
DZ_SKIP_CAP = 1e-3


@functools.lru_cache(maxsize=None)
def backward_case(shape):
    """z is an INPUT of the block (fp32), so the float64 reference differentiates BatchNorm + ReLU from the same z: nothing depends on
    a convolution's rounding.  The first seed whose float64 pre-ReLU values all stay MASK_EXACT away from zero is taken (a flipped
    mask element moves dbeta by a whole dy, far beyond any bar): a property of the reference alone."""
    B, H, W, Cin, Cout = shape
    a = 0.9 * float(np.sqrt(6.0 / (9 * Cin)))
    for seed in range(50):
        x = torch.from_numpy(O.formula_normal("tb/bwd/x", (B, Cin, H, W), seed=seed))
        w = torch.from_numpy(O.formula_uniform("tb/bwd/w", (Cout, Cin, 3, 3), -a, a, seed=seed))
        b = torch.from_numpy(O.formula_uniform("tb/bwd/b", (Cout,), -0.1, 0.1, seed=seed))
        z = F.conv2d(x.double(), w.double(), b.double(), padding=1).float()
        gamma = torch.from_numpy(O.formula_uniform("tb/bwd/gamma", (Cout,), 0.5, 1.5, seed=seed))
        gamma[::3] *= -1                                   # negative gammas flip the sign test of the recomputed ReLU mask
        beta = torch.from_numpy(O.formula_uniform("tb/bwd/beta", (Cout,), -0.5, 0.5, seed=seed))
        zd, gd, bd = z.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
        pre = F.batch_norm(zd, None, None, gd, bd, training=True, momentum=MOM, eps=EPS)
        if float(pre.detach().abs().min()) >= MASK_EXACT:
            break
    else:
        raise RuntimeError("no seed keeps the float64 pre-ReLU values away from zero")
    dy = torch.from_numpy(O.formula_normal("tb/bwd/dy", (B, Cout, H, W), seed=seed + 1))
    F.relu(pre).backward(dy.double())
    dz = zd.grad
    mean, var = z.double().mean((0, 2, 3)), z.double().var((0, 2, 3), unbiased=False)
    ref = {"dz": dz, "dgamma": gd.grad, "dbeta": bd.grad, "pre": pre.detach(),
           "dw": torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), dz, padding=1),
           "din": torch.nn.grad.conv2d_input((B, Cin, H, W), w.double(), dz, padding=1)}
    inp = {"x": x, "w": w, "z": z, "dy": dy, "gamma": gamma, "beta": beta, "mean": mean.float(), "invstd": (1.0 / torch.sqrt(var + EPS)).float()}
    return inp, ref


def run_backward(cuda, ctx, inp, pad_dy=4):
    x, w, z, dy = inp["x"], inp["w"], inp["z"], inp["dy"]
    B, Cin, H, W = x.shape
    Cout, Cp = w.shape[0], (Cin + 3) // 4 * 4
    ld_dy = Cout + pad_dy
    xin = torch.zeros((B, H, W, Cp), device=cuda)
    xin[..., :Cin] = nhwc(x).to(cuda)
    dyb = torch.full((B, H, W, ld_dy), 3.0, device=cuda)       # channels beyond Cout: unrelated data that must not be read
    dyb[..., :Cout] = nhwc(dy).to(cuda)
    zc, wd = nhwc(z).to(cuda), w.contiguous().to(cuda)
    par = {k: inp[k].to(cuda) for k in ("gamma", "beta", "mean", "invstd")}
    o = {"dz": torch.full((B, H, W, Cout), float("nan"), device=cuda), "dw": torch.full((Cout, Cin, 3, 3), float("nan"), device=cuda),
         "din": torch.full((B, H, W, Cin), float("nan"), device=cuda)}
    o.update({k: torch.full((Cout,), float("nan"), device=cuda) for k in ("dgamma", "dbeta", "dbias")})
    _lib.check(_lib.lib().mgu_bn_relu_conv_backward_nhwc(
        ctx.handle, xin.data_ptr(), Cp, zc.data_ptr(), dyb.data_ptr(), ld_dy, par["gamma"].data_ptr(), par["beta"].data_ptr(),
        par["mean"].data_ptr(), par["invstd"].data_ptr(), wd.data_ptr(), B, H, W, Cin, Cout, o["dz"].data_ptr(), o["dgamma"].data_ptr(),
        o["dbeta"].data_ptr(), o["dbias"].data_ptr(), o["dw"].data_ptr(), o["din"].data_ptr(), Cin, _lib.current_stream_ptr(cuda)), ctx.handle)
    torch.cuda.synchronize()
    return o


def chan_reduce_terms(M, C):
    """fp32 terms one thread of chan_reduce_kernel accumulates (launch_chan_reduce, train_kernels.hip): <= 512 workgroups of `rows`
    pixel rows each, 256 / (C / 4) row lanes per workgroup."""
    blocks = min((M + 63) // 64, 512)
    rows = (M + blocks - 1) // blocks
    npl = 256 // (C // 4)
    return (rows + npl - 1) // npl


@pytest.mark.parametrize("variant", list(BWD_ENVS))
@pytest.mark.parametrize("shape", BWD_CASES)
def test_backward_block_vs_float64(cuda, variant, shape):
    B, H, W, Cin, Cout = shape
    inp, ref = backward_case(shape)
    near = ref["pre"].abs() < DZ_SKIP
    assert float(near.double().mean()) <= DZ_SKIP_CAP
    with context(cuda, **BWD_ENVS[variant]) as ctx:
        o = run_backward(cuda, ctx, inp)
    dz = o["dz"].permute(0, 3, 1, 2).double().cpu()
    # the ReLU mask the kernel recomputed, recovered from its dz: dz = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy or 0
    M = B * H * W
    zd = inp["z"].double()
    mean, var = zd.mean((0, 2, 3)), zd.var((0, 2, 3), unbiased=False)
    istd = 1.0 / torch.sqrt(var + EPS)
    v = lambda t: t.view(1, -1, 1, 1)
    xhat = (zd - v(mean)) * v(istd)
    g = dz / v(inp["gamma"].double() * istd) + v(ref["dbeta"]) / M + xhat * v(ref["dgamma"]) / M
    dyd = inp["dy"].double()
    live = dyd.abs() > 1e-3
    mask_gpu, mask_ref = (g - dyd).abs() < g.abs(), ref["pre"] > 0
    flips = live & (mask_gpu != mask_ref)
    assert not bool((flips & (ref["pre"].abs() >= MASK_EXACT)).any()), int(flips.sum())
    scale = float(ref["dz"].abs().max())
    e = {"dz": float(((dz - ref["dz"]).abs() * (~near)).max()) / scale, "dgamma": rel(o["dgamma"], ref["dgamma"]), "dbeta": rel(o["dbeta"], ref["dbeta"]),
         "dw": rel(o["dw"], ref["dw"]), "din": rel(o["din"].permute(0, 3, 1, 2), ref["din"])}
    # the conv bias in front of a BatchNorm has an analytically zero gradient; what the fold must produce is the column sum of the
    # kernel's own fp32 dz, to within the fp32 accumulation of a thread's k terms (the rows then meet in double)
    col, colabs = dz.sum((0, 2, 3)), dz.abs().sum((0, 2, 3))
    k = chan_reduce_terms(M, Cout)
    db = float(((o["dbias"].double().cpu() - col).abs() / (k * 2.0 ** -24 * colabs)).max())
    print(f"[train-block bwd {shape}/{variant}] " + " ".join(f"{n} {x:.2e}" for n, x in e.items()) + f" dbias/bound {db:.3f} (k = {k})")
    assert all(v <= TOL for v in e.values()), e   # (every entry: a NaN fails its own comparison)
    assert db <= 1.0, db


# ---- (c) slot hygiene ---------------------------------------------------------------------------------------------------------------
def slots_absmax(cuda, ctx):
    v = C.c_double(-1.0)
    _lib.check(_lib.lib().mgu_reduction_slots_absmax(ctx.handle, C.byref(v), _lib.current_stream_ptr(cuda)), ctx.handle)
    return v.value


def test_reduction_slots_are_clean_between_blocks(cuda):
    """One adder per table element onto zero: a block's results cannot depend on what ran before it in the context.  A sequence
    that changes the table's pitch (2 * C doubles per row) and its row count from call to call, each call bit-identical to the same
    call made first in a fresh context; afterwards the whole table is zero."""
    steps = [("fwd", plain_case("wide_even")[0]), ("bwd", backward_case(BWD_CASES[1])[0]), ("fwd", plain_case("three_n_blocks")[0]),
             ("fwd", plain_case("three_n_blocks")[0]), ("fwd", plain_case("direct_cin8")[0]), ("bwd", backward_case(BWD_CASES[3])[0])]
    run = lambda ctx, kind, inp: run_forward(cuda, ctx, inp) if kind == "fwd" else run_backward(cuda, ctx, inp)
    fresh = []
    for kind, inp in steps:
        with context(cuda) as ctx:
            fresh.append(run(ctx, kind, inp))
            assert slots_absmax(cuda, ctx) == 0.0
    assert [o.get("stats_fused") for o in fresh] == [1, None, 1, 1, 0, None]
    with context(cuda) as ctx:
        for rnd in range(2):   # the second round finds the table at its final size: no reallocation clears it on the way
            for i, (kind, inp) in enumerate(steps):
                o = run(ctx, kind, inp)
                for k, t in o.items():
                    if isinstance(t, torch.Tensor):
                        assert torch.equal(t, fresh[i][k]), (rnd, i, kind, k)
        assert slots_absmax(cuda, ctx) == 0.0
