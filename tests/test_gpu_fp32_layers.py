"""The fp32 eval forward form by form: every case of fp32_oracle.CASES is an fp32 mgunet.UNet whose widths, class count and input
channels put layers on kernel forms the shipped 8 / 12 / 16 / 32-feature networks never reach as a network (C++ component-pair Winograd
with odd chunk counts and N tails, the assembly forms next to them, tile kernels feeding Winograd layers, both ConvTranspose kernels,
the first-convolution forms, the head and patch-mean passes at every class count, the direct halo kernel), below one patch, ragged
with odd levels, and on whole patch grids.  Every (case, size) runs in a fresh model with a patch-mean request at patch 16

  a. with formula weights under the per-element bars of fp32_oracle.judge (float64 segment references computed from the HIP path's own
     exposed tensors; c measured at test time on two CPU fp32 emulations, never on the kernels), the concat buffers' up-sampled halves
     against the float64 ConvTranspose with their pad rows exactly zero;
  b. with exact data under torch.equal (fp32_oracle: why the forward is exact there), NCHW and channels_last, every seed, twice;
  c. and proves from the profiling records that the launches are the ones fp32_oracle.family_launches derives.

Figures of one MI355X run: NOTES.md, "fp32 forward, form by form"."""
import pytest
import torch
import torch.nn.functional as F

import fp32_oracle as P
import mgunet
import mgunet_oracle as O
from mgunet import _lib

pytestmark = pytest.mark.gpu

MATRIX = [(case, size) for case in P.CASES for size in P.sizes(case)]


def model(case, p, cuda, monkeypatch):
    """A fresh eval model whose context was created under the case's switches."""
    sw = P.SWITCHES.get(case, {})
    for k in ("MGU_WINO_ASM", "MGU_WINO_PREC", "MGU_NO_WINOGRAD", "MGU_NO_WINO_CP", "MGU_NO_CONVT_FRAG", "MGU_HEAD_FUSED", "MGU_NO_FIRST_MFMA"):
        monkeypatch.delenv(k, raising=False)
    for k, v in sw.items():
        monkeypatch.setenv(k, v)
    m = mgunet.UNet(*P.CASES[case][0])
    m.load_state_dict(p)
    m = m.to(cuda).eval()
    m._context(cuda)
    for k in sw:
        monkeypatch.delenv(k)
    return m


def forward(m, x, profile=False):
    """One forward with a patch-mean request: ((logits, skips, feats, patch means), concat buffers, {record: launches})."""
    dev = x.device
    Bn, _, H, W = x.shape
    ctx, L = m._context(dev), _lib.lib()
    pm = torch.full((Bn * (-(-H // P.PATCH)) * (-(-W // P.PATCH)), m.init_features), float("nan"), device=dev)
    launched = None
    with torch.no_grad():
        if profile:
            _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
        _lib.call("mgu_unet_request_patch_mean", dev, P.PATCH, pm, ctx=ctx)
        lg, sk, ft = m(x)
        torch.cuda.synchronize(dev)
        if profile:
            launched = {k["name"]: k["launches"] for k in _lib.read_kernel_stats(ctx)}
            _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return (lg, sk, ft, pm), [s._base for s in sk], launched


def check_up_halves(p64, depth, cats, ft, tag):
    """Channels [C, 2C) of concat buffer i: zero in the pad rows / columns of an odd level, elsewhere the float64 ConvTranspose of the
    path's own feature i + 1 within 2e-6 * (sum |x w| + |b|) (one layer of the conv bar)."""
    for i in range(depth):
        cat = cats[i].double().cpu().permute(0, 3, 1, 2)
        C = cat.shape[1] // 2
        up, (H, W) = cat[:, C:], cat.shape[2:]
        h, w = 2 * (H // 2), 2 * (W // 2)
        assert not up[:, :, h:].any() and not up[:, :, :, w:].any(), (tag, f"concat {i}: a pad row / column is not zero")
        if i == depth - 1:
            continue          # (its source, the bottleneck, is not exposed: the deep segment covers it)
        wt, b = p64[f"decoder.decoder_blocks.{depth - 1 - i}.upsample.weight"], p64[f"decoder.decoder_blocks.{depth - 1 - i}.upsample.bias"]
        with torch.no_grad():
            ref = F.conv_transpose2d(ft[i + 1].double().cpu(), wt, b, stride=2)
            S = F.conv_transpose2d(ft[i + 1].double().cpu().abs(), wt.abs(), b.abs(), stride=2)
        worst, share = P.worst_ratio(up[:, :, :h, :w], ref, P.C_FLOOR * S)
        print(f"    [{tag}] concat {i} up-sampled half: worst / bar {worst:.3f}, mismatch {share * 100:.2f} %")
        assert worst <= 1.0, (tag, i, worst)


@pytest.mark.parametrize("case,size", MATRIX)
def test_formula_weights_under_the_per_element_bar(cuda, monkeypatch, case, size):
    cfg = P.CASES[case][0]
    depth = cfg[3]
    shape = P.sizes(case)[size]
    p = O.make_unet_params(*cfg, seed=21)
    x = torch.from_numpy(O.formula_normal(f"fp32layers/{case}/x", shape, seed=21))
    m = model(case, p, cuda, monkeypatch)
    forward(m, x.to(cuda))                                   # (weights packed, workspace sized)
    got, cats, launched = forward(m, x.to(cuda), profile=True)
    want = P.family_launches(cfg, shape, P.SWITCHES.get(case))
    print(f"    [{case} {size}] launched {launched}\n    [{case} {size}] predicted {want}")
    assert launched == want, (case, size, launched, want)
    lg, sk, ft, pm = got
    assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in [lg, pm] + sk + ft)
    p64 = P.f64_params(p)
    cpu = (lg.cpu(), [t.cpu() for t in sk], [t.cpu() for t in ft], pm.cpu())
    fig = P.judge(p64, depth, x, cpu, f"{case} {size}")
    check_up_halves(p64, depth, cats, ft, f"{case} {size}")
    assert not P.misses(fig), (case, size, P.misses(fig), fig)


@pytest.mark.parametrize("case", list(P.CASES))
def test_exact_data_bit_for_bit(cuda, monkeypatch, case):
    """Small-integer data on which the fp32 forward has exactly one right answer (fp32_oracle: the exactness argument): every index
    mapping of every kernel form -- pixel, channel, tap, chunk, N tile, pool window, quadrant, pad row, head lane, patch -- must come out
    bit for bit, at every size and for every seed of exact_seeds (after which every (tap, cin) position of every layer has been
    nonzero)."""
    cfg = P.CASES[case][0]
    depth = cfg[3]
    szs = list(P.sizes(case).items())
    runs = [(seed, s) for seed in range(P.exact_seeds(cfg)) for s in szs]
    m = None
    for seed, (size, shape) in runs:
        p = P.exact_params(cfg, seed)
        if m is None:
            m = model(case, p, cuda, monkeypatch)
        else:
            m.load_state_dict(p)
        x = P.exact_input(shape, seed)
        ref = P.exact_reference(p, x, depth)
        for layout in ("nchw", "channels_last"):
            xg = x.to(cuda)
            if layout == "channels_last":
                xg = xg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            got, _, _ = forward(m, xg)
            again, _, _ = forward(m, xg)
            bad = P.differing(got, ref)
            assert not bad, (case, seed, size, layout, bad, _where(got, ref, bad[0]))
            flat = lambda o: [o[0]] + o[1] + o[2] + [o[3]]
            assert all(torch.equal(a, b) for a, b in zip(flat(got), flat(again))), (case, seed, size, layout, "a second call returns other bytes")


def _where(got, ref, name):
    """Where the failing tensor differs: count, channel range and the first positions."""
    pick = lambda o: o[0] if name == "logits" else o[3] if name == "patch_means" else o[1 if name.startswith("skip") else 2][int(name[4:])]
    g, r = pick(got).double().cpu(), pick(ref)
    bad = (g != r).nonzero()
    return f"{name}: {bad.shape[0]} of {r.numel()} differ; channels {int(bad[:, 1].min())}..{int(bad[:, 1].max())}; first {bad[:4].tolist()}"
