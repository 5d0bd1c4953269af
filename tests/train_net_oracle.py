"""The U-Net training step with its decisions pinned, for tests/test_train_net_host.py (CPU) and tests/test_gpu_train_net.py (GPU).

Train-mode BatchNorm, ReLU and MaxPool make the network gradient discontinuous in the forward's rounding: a float64 reference that makes
its own ReLU and arg-max decisions sits 1-5 % away from any fp32 path as soon as ONE decision among a million differs.  The reference
here decides nothing.  pinned_network is mgunet_oracle.unet_forward in train mode (batch statistics, eps 1e-5, skip first in the
concat, trailing pad) with
    y = bn(z) * mask          mask = pins[layer], the path's own y > 0
    MaxPool = a gather        at pins["pool{i}"], the indices F.max_pool2d(y, 2, return_indices=True) gives on the path's own fp32
                              skip (the first maximum wins: the rule include/mgunet.h documents for mgu_maxpool2x2_backward_nhwc)
so that it is a smooth function of the parameters and every gradient of the path can be held to the kernels' own bar.  What the pins
leave open -- that the path's decisions are the right ones -- is checked against free_decisions, the float64 network's own, with the
project's margins for a ReLU at its kink and a pool window near a tie.

The bars (judge).  For every parameter tensor t but the conv biases under BatchNorm
    max |g_t - ref_t| / max |ref_t| <= bar_t = max(TOL, C_FACTOR * the larger error on t of the two CPU fp32 emulations)
ref = the pinned float64 network, the emulations the same pinned network in torch fp32, contiguous and channels_last (two summation
orders); TOL = 2e-5 is the isolated backward kernels' bar (tests/test_gpu_backward_kernels.py), C_FACTOR the project's `4 * cond`.
bar_t never sees a kernel.  A conv bias under BatchNorm has an analytically zero gradient: |g_c| <= 1e-4 * sum |dz_c| over the
reference's z.grad (the bound of test_bn_relu_forward_backward_vs_float64).

MUTANTS are wrong backward schedules expressed in the reference (the forward's values are the right ones, the gradient is the one the
wrong schedule would produce); backward_launches restates pick_wgrad (csrc/wgrad_f32.hip), the data-gradient pick of conv_dgrad and
the ConvTranspose data-gradient pick of convt_dgrad (csrc/mgunet_train.hip, csrc/igemm.hip) for the profiling-record names of one
mgu_unet_backward."""
import torch
import torch.nn.functional as F

import fp32_oracle as P
import mgunet_oracle as O
from fp32_oracle import C_FACTOR, f64_params  # noqa: F401  (shared, not copied)

TOL = 2e-5               # tests/test_gpu_backward_kernels.py TOL: the isolated backward kernels' bar, relative to the result's max
RELU_MARGIN = 1e-5       # tests/test_gpu_train_blocks.py DZ_SKIP: a ReLU decision may differ from float64's only this close to the kink
POOL_MARGIN = 5e-5       # tests/test_gpu_train.py well_posed_case: a pool index may differ only where float64's top two are this close
DIFFER_CAP = 1e-4        # share of decisions that may differ from float64's at all (a condition; the CPU stand-in stays below 3e-6)
BIAS_BOUND = 1e-4        # conv bias under BatchNorm: |g_c| <= BIAS_BOUND * sum |dz_c|
EPS = 1e-5

# ---- the cases ----------------------------------------------------------------------------------------------------------------------
# fp32_oracle's configurations under their switches, a network with five classes and five input channels (the head through run_layer
# with ldd = 8, Cp0 = 8), and two networks under the A/B switches of tests/test_gpu_backward_kernels.py (MGU_NO_WGRAD_X3 is there
# for the fp32-MFMA Winograd weight gradient, which no other switch reaches).
CASES = {name: (cfg, dict(P.SWITCHES.get(name, {}))) for name, (cfg, _) in P.CASES.items()}
CASES["f8d2c5i5"] = ((5, 5, 8, 2), {})
for _tag, _cfg in (("f32d2", (3, 2, 32, 2)), ("f64d1", (3, 2, 64, 1))):
    for _sw, _v in (("MGU_NO_WINO_WGRAD", "1"), ("MGU_NO_WINO_DGRAD", "1"), ("MGU_NO_CONVT_DGRAD_X3", "1"), ("MGU_WINO_PREC", "0")):
        CASES[f"{_tag}_{_sw[4:].lower()}"] = (_cfg, {_sw: _v})
CASES["f32d2_no_wgrad_x3"] = ((3, 2, 32, 2), {"MGU_NO_WGRAD_X3": "1"})
SWITCH_NAMES = ("MGU_NO_WINOGRAD", "MGU_WINO_PREC", "MGU_NO_WINO_CP", "MGU_NO_WGRAD_HALO", "MGU_NO_WINO_WGRAD", "MGU_NO_WGRAD_X3",
                "MGU_NO_CONVT_DGRAD_X3", "MGU_NO_THIN_WGRAD", "MGU_NO_WINO_DGRAD", "MGU_NO_CONVT_FRAG")


def sizes(case):
    """fp32_oracle.sizes: small 2 x C x 12 x 20, ragged 2 x C x 50 x 70, whole 1 x C x 64 x 96 (128 wide for f96d1); no small at depth 3."""
    if case in P.CASES:
        return P.sizes(case)
    cin, depth = CASES[case][0][0], CASES[case][0][3]
    like = {1: "f80d1", 2: "f24d2"}[depth]                       # the added cases: the sizes of a shared case of the same depth
    return {k: (s[0], cin) + s[2:] for k, s in P.sizes(like).items()}


# ---- layer names ----------------------------------------------------------------------------------------------------------------------
def block_prefixes(depth):
    """ConvBlock prefixes in forward order: encoder blocks, bottleneck, decoder blocks."""
    return [f"encoder.encoder_blocks.{i}." for i in range(depth)] + ["encoder.bottleneck."] + \
        [f"decoder.decoder_blocks.{b}.conv_block." for b in range(depth)]


def bn_layers(depth):
    """The conv -> BatchNorm -> ReLU layers by state_dict prefix, forward order."""
    return [pre + c for pre in block_prefixes(depth) for c in ("conv1", "conv2")]


def other_layers(depth):
    """The layers that record their input only."""
    return [f"decoder.decoder_blocks.{b}.upsample" for b in range(depth)] + ["decoder.final_conv"]


def bn_of(layer):
    return layer[:-5] + "bn" + layer[-1]           # "....conv1" -> "....bn1"


def is_bn_conv_bias(name):
    return name.endswith("conv1.bias") or name.endswith("conv2.bias")


# ---- the pinned network -----------------------------------------------------------------------------------------------------------------
MUTANTS = ("upconv_bias_grad_over_pad", "pad_leading", "pool_backward_overwrites", "dcat_halves_swapped", "conv1_mask_from_conv2",
           "bn_param_grads_unmasked")


class _CatSwappedGrad(torch.autograd.Function):
    """torch.cat([a, b], 1) whose backward hands each input the other half of d(cat)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.c = a.shape[1]
        return torch.cat([a, b], 1)

    @staticmethod
    def backward(ctx, g):
        return g[:, ctx.c:].contiguous(), g[:, :ctx.c].contiguous()


class Run:
    """One evaluation: logits, the leaf parameters q (name -> tensor with .grad after backward), z of every conv -> BN layer (retained
    for z.grad), the decisions it used -- made (pins None) or given: mask[layer], pre[layer] (the pre-ReLU value), pool{i} -- and
    record[layer] = {in, z, y, mean, invstd}, what a path's train-forward record holds of a conv -> BN layer."""

    def __init__(self):
        self.logits, self.q, self.z, self.mask, self.pre, self.pool, self.record = None, {}, {}, {}, {}, {}, {}


def _half_block(run, q, layer, x, pins, mutant):
    z = F.conv2d(x, q[layer + ".weight"], q[layer + ".bias"], padding=1)
    if z.requires_grad:
        z.retain_grad()
    run.z[layer] = z
    mean = z.mean((0, 2, 3), keepdim=True)
    var = z.var((0, 2, 3), unbiased=False, keepdim=True)
    xh = (z - mean) * torch.rsqrt(var + EPS)
    g, b = q[bn_of(layer) + ".weight"].view(1, -1, 1, 1), q[bn_of(layer) + ".bias"].view(1, -1, 1, 1)
    a = xh * g + b
    m = (a > 0) if pins is None else pins[layer]
    run.mask[layer], run.pre[layer] = m, a.detach()
    mt = m.to(a.dtype)
    if mutant == "conv1_mask_from_conv2" and layer.endswith("conv1"):
        mw = pins[layer[:-1] + "2"].to(a.dtype)
        y = a * mw + (a * mt - a * mw).detach()                      # the value of the right mask, the gradient of the wrong one
    elif mutant == "bn_param_grads_unmasked":
        free = xh.detach() * g + b                                   # gamma / beta see every element, z only the live ones
        y = (xh * g.detach() + b.detach()) * mt + (free - free.detach())
    else:
        y = a * mt
    run.record[layer] = {"in": x.detach(), "z": z.detach(), "y": y.detach(), "mean": mean.detach().flatten(),
                         "invstd": torch.rsqrt(var + EPS).detach().flatten()}
    return y


def _block(run, q, pre, x, pins, mutant):
    return _half_block(run, q, pre + "conv2", _half_block(run, q, pre + "conv1", x, pins, mutant), pins, mutant)


def _pool(run, key, y, pins):
    idx = F.max_pool2d(y.detach(), 2, return_indices=True)[1] if pins is None else pins[key]
    run.pool[key] = idx
    return y.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)


def pinned_network(p, x, depth, pins, dtype, mutant=None, channels_last=False):
    """The train-mode forward in `dtype` on leaf copies of the parameters p.  pins: {layer: bool mask, "pool{i}": indices}; None: the
    network decides itself (and Run records what it decided).  mutant: one of MUTANTS."""
    assert mutant is None or (mutant in MUTANTS and pins is not None)
    run = Run()
    q = run.q = {k: v.to(dtype).clone().requires_grad_() for k, v in p.items() if v.dtype.is_floating_point and "running" not in k}
    cur = x.to(dtype)
    if channels_last:
        cur = cur.contiguous(memory_format=torch.channels_last)
    skips = []
    for i in range(depth):
        cur = _block(run, q, f"encoder.encoder_blocks.{i}.", cur, pins, mutant)
        skips.append(cur)
        cur = _pool(run, f"pool{i}", cur, pins)
    cur = _block(run, q, "encoder.bottleneck.", cur, pins, mutant)
    for bi in range(depth):
        skip = skips[depth - 1 - bi]
        pre = f"decoder.decoder_blocks.{bi}."
        w, b = q[pre + "upsample.weight"], q[pre + "upsample.bias"]
        up = F.conv_transpose2d(cur, w, b, stride=2)
        dy, dx = skip.shape[2] - up.shape[2], skip.shape[3] - up.shape[3]
        pad = [dx - dx // 2, dx // 2, dy - dy // 2, dy // 2] if mutant == "pad_leading" else [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2]
        up = F.pad(up, pad)
        if mutant == "upconv_bias_grad_over_pad":                    # the bias column sums taken before the pad region is zeroed
            bb = b.view(1, -1, 1, 1).expand_as(up)
            up = F.pad(F.conv_transpose2d(cur, w, b.detach(), stride=2), pad) + (bb - bb.detach())
        if mutant == "pool_backward_overwrites":                     # the decoder-side gradient of the skip is lost wherever a pool
            tail = torch.zeros_like(skip, dtype=torch.bool)          # window lies (an odd level's last row / column keeps it)
            tail[:, :, skip.shape[2] // 2 * 2:] = True
            tail[:, :, :, skip.shape[3] // 2 * 2:] = True
            skip = torch.where(tail, skip, skip.detach())
        cat = _CatSwappedGrad.apply(skip, up) if mutant == "dcat_halves_swapped" else torch.cat([skip, up], 1)
        cur = _block(run, q, pre + "conv_block.", cat, pins, mutant)
    run.logits = F.conv2d(cur, q["decoder.final_conv.weight"], q["decoder.final_conv.bias"])
    return run


def gradients(p, x, dlogits, depth, pins, dtype, mutant=None, channels_last=False):
    """(parameter gradients, z.grad of every conv -> BN layer, the Run), float64 out, of pinned_network for d(loss)/d(logits) = dlogits
    (B, classes, H, W)."""
    run = pinned_network(p, x, depth, pins, dtype, mutant, channels_last)
    run.logits.backward(dlogits.to(dtype))
    return {k: v.grad.double() for k, v in run.q.items()}, {k: z.grad.double() for k, z in run.z.items()}, run


def pins_of(run):
    return {**run.mask, **run.pool}


def pins_from(record, depth):
    """The pins from the copied-out y tensors of a path: record[layer]["y"] (B, C, H, W) fp32 of every conv -> BN layer."""
    pins = {layer: record[layer]["y"] > 0 for layer in bn_layers(depth)}
    for i in range(depth):
        pins[f"pool{i}"] = F.max_pool2d(record[f"encoder.encoder_blocks.{i}.conv2"]["y"].float(), 2, return_indices=True)[1]
    return pins


def record_ratios(p64, record, depth):
    """A path's forward record against float64 of its OWN tensors, as error / bar: per conv -> BN layer z against the float64
    convolution of the recorded input, per element within C_FLOOR * (sum |x w| + |b|), and mean / invstd against the float64
    statistics of the recorded z within TOL of the largest."""
    out = {}
    with torch.no_grad():
        for layer in bn_layers(depth):
            r, w, b = record[layer], p64[layer + ".weight"], p64[layer + ".bias"]
            xin = r["in"].double()
            ref = F.conv2d(xin, w, b, padding=1)
            S = F.conv2d(xin.abs(), w.abs(), b.abs(), padding=1)
            out[layer + " z"] = P.worst_ratio(r["z"], ref, P.C_FLOOR * S)[0]
            z = r["z"].double()
            stats = {"mean": z.mean((0, 2, 3)), "invstd": torch.rsqrt(z.var((0, 2, 3), unbiased=False) + EPS)}
            for k, want in stats.items():
                out[f"{layer} {k}"] = float((r[k].double() - want).abs().max()) / float(want.abs().max()) / TOL
    return out


def free_decisions(p64, x, depth):
    """The float64 network's own decisions: (pins, pre-ReLU value per layer, top-2 gap per pool window)."""
    with torch.no_grad():
        run = pinned_network(p64, x, depth, None, torch.float64)
    gaps = {}
    for i in range(depth):
        y = run.record[f"encoder.encoder_blocks.{i}.conv2"]["y"]
        B, C, H, W = y.shape
        win = y[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
        top = win.topk(2, dim=-1).values
        gaps[f"pool{i}"] = top[..., 0] - top[..., 1]
    return pins_of(run), run.pre, gaps


def compare_decisions(pins, free):
    """The path's pins against free_decisions: (decisions, differing, differing outside the margins [(key, count)])."""
    fp, pre, gaps = free
    total = differing = 0
    outside = []
    for key, mine in pins.items():
        d = mine != fp[key]
        far = d & ((gaps[key] > POOL_MARGIN) if key.startswith("pool") else (pre[key].abs() > RELU_MARGIN))
        total += d.numel()
        differing += int(d.sum())
        if bool(far.any()):
            outside.append((key, int(far.sum())))
    return total, differing, outside


# ---- the bars -------------------------------------------------------------------------------------------------------------------------
def rel_errors(g, ref):
    """max |g - ref| / max |ref| per parameter tensor (the conv biases under BatchNorm left to bias_ratios)."""
    return {k: float((g[k].double() - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-300) for k in ref if not is_bn_conv_bias(k)}


def reference(p, x, dlogits, depth, pins):
    """(ref gradients, ref z.grad, bar per tensor, the two emulations' errors) for the pins of a path."""
    ref, dz, _ = gradients(p, x, dlogits, depth, pins, torch.float64)
    emu = {"fp32": rel_errors(gradients(p, x, dlogits, depth, pins, torch.float32)[0], ref),
           "fp32_channels_last": rel_errors(gradients(p, x, dlogits, depth, pins, torch.float32, channels_last=True)[0], ref)}
    bar = {k: max(TOL, C_FACTOR * max(e[k] for e in emu.values())) for k in emu["fp32"]}
    return ref, dz, bar, emu


def bias_ratios(g, dz):
    """worst |g_c| / (BIAS_BOUND * sum |dz_c|) per conv bias under BatchNorm."""
    return {layer + ".bias": float((g[layer + ".bias"].double().abs() / (BIAS_BOUND * d.abs().sum((0, 2, 3))).clamp_min(1e-300)).max())
            for layer, d in dz.items()}


def judge(g, ref, dz, bar, tag="", show=print):
    """{tensor: error / bar} of a path's gradients g; a ratio above 1 misses its bar."""
    ratio = {k: e / bar[k] for k, e in rel_errors(g, ref).items()}
    ratio.update(bias_ratios(g, dz))
    k = max(ratio, key=lambda n: ratio[n] if ratio[n] == ratio[n] else float("inf"))
    show(f"    [{tag}] worst error / bar {ratio[k]:.3f} on {k} (bar {bar.get(k, BIAS_BOUND):.2e})")
    return ratio


def misses(ratio):
    return sorted(k for k, r in ratio.items() if not r <= 1.0)


def formula_dlogits(tag, shape, ncls):
    """(npix, rup(ncls, 4)) fp32 with zero pad columns as mgu_unet_backward reads it, and the same values as (B, ncls, H, W): dense
    formula values / npix, so that every class column carries a signal of its own."""
    Bn, _, H, W = shape
    npix = Bn * H * W
    v = torch.from_numpy(O.formula_normal(tag + "/dlogits", (npix, ncls), seed=22)) / npix
    padded = torch.zeros((npix, -(-ncls // 4) * 4), dtype=torch.float32)
    padded[:, :ncls] = v
    return padded, v.reshape(Bn, H, W, ncls).permute(0, 3, 1, 2).contiguous()


# ---- the launches of one backward -----------------------------------------------------------------------------------------------------
WGRAD_THIN, WGRAD_WINO_X3, WGRAD_WINO, WGRAD_DIRECT = ("wgrad_thin kernels", "wino_wgrad_f32_kernel<X3>", "wino_wgrad_f32_kernel",
                                                       "wgrad (direct) kernels")
DGRAD_TILES, CONVT_DGRAD_X3, CONVT_DGRAD_TILES = "igemm/halo (dgrad)", "convt2x2_x3_kernel (dgrad)", "igemm_kernel<f32> (ConvTranspose dgrad)"
DGRAD_WINO = ("wino3x3_cp_kernel<1> (dgrad)", "wino3x3_cp_kernel<2> (dgrad)", "wino3x3_f32_kernel<*,1> (dgrad)", "wino3x3_f32_kernel<*,0> (dgrad)")


def _rup(v, m):
    return -(-v // m) * m


def _wgrad_name(M, cp, n, sw):
    """pick_wgrad on a 3x3 layer of the network walk (pitches multiples of 4, the partial-panel scratch large enough)."""
    if not sw.get("MGU_NO_THIN_WGRAD") and M >= 4096 and n == 32 and cp == 4:
        return WGRAD_THIN
    if cp % 32 == 0 and n % 32 == 0 and not sw.get("MGU_NO_WINO_WGRAD"):
        return WGRAD_WINO if sw.get("MGU_NO_WGRAD_X3") else WGRAD_WINO_X3
    return WGRAD_DIRECT


def _dgrad_name(cin, cp, cop, sw):
    """conv_dgrad's pick: the Winograd kernel where the layer keeps a data-gradient set (weight_forms: wino_layer on Cp and on Cop)."""
    prec = int(sw.get("MGU_WINO_PREC", "1")) != 0
    if sw.get("MGU_NO_WINOGRAD") or sw.get("MGU_NO_WINO_DGRAD") or cp % 16 or cop % 16:
        return DGRAD_TILES
    if not prec:
        return DGRAD_WINO[3]
    if sw.get("MGU_NO_WINO_CP"):
        return DGRAD_WINO[2]
    return DGRAD_WINO[1] if cin > 32 else DGRAD_WINO[0]


def _convt_dgrad_name(cin, cout, sw):
    prec = int(sw.get("MGU_WINO_PREC", "1")) != 0
    return CONVT_DGRAD_X3 if prec and not sw.get("MGU_NO_CONVT_DGRAD_X3") and cin % 64 == 0 and cout % 32 == 0 else CONVT_DGRAD_TILES


def backward_launches(cfg, shape, switches=None):
    """Profiling-record name -> launches of one mgu_unet_backward: a weight gradient per conv -> BN layer, a data gradient per such
    layer but the first, a ConvTranspose data gradient per decoder block (the head's and the ConvTranspose weight gradients carry no
    record)."""
    sw = switches or {}
    cin0, _, f, depth = cfg
    Bn, _, H, W = shape
    out = {}

    def add(name):
        out[name] = out.get(name, 0) + 1

    def block(cin, cout, lvl, first=False):
        M = Bn * (H >> lvl) * (W >> lvl)
        for i, ci in enumerate((cin, cout)):
            cp = _rup(ci, 4)
            add(_wgrad_name(M, cp, _rup(cout, 4), sw))
            if not (first and i == 0):
                add(_dgrad_name(ci, cp, _rup(cout, 4), sw))

    cin = cin0
    for i in range(depth):
        block(cin, f << i, i, first=i == 0)
        cin = f << i
    block(cin, f << depth, depth)
    for i in reversed(range(depth)):
        add(_convt_dgrad_name(2 * (f << i), f << i, sw))
        block(2 * (f << i), f << i, i)
    return out
