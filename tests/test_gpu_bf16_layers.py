"""The bf16-storage kernels form by form: every case of bf16_oracle.CASES is a bf16 mgunet.UNet whose channel widths put layers on
kernel forms the shipped 8 / 16 / 32-feature networks never reach (odd chunk counts, N tails, K tails, the generic ConvTranspose at
other widths, the first-convolution forms), on sizes smaller than a patch, ragged against both patch shapes with odd levels below,
whole patch grids, and one large enough that a halo workgroup walks several patches.  Each case runs

  * with formula weights (O.make_unet_params) under the per-element bar of bf16_oracle.check: every exposed tensor against the float64
    segment reference computed from the HIP path's own exposed predecessors; the fp32 logits against the fp32 head on the bf16 feature;
  * with exact data (bf16_oracle.exact_params / exact_input) under torch.equal on every exposed tensor, NCHW and channels_last input,
    every seed, and a second call returning the same bytes;

and proves from the profiling records that the kernel families its row of the table claims were launched, as often as
bf16_oracle.layer_forms derives from (Cp, N)."""
import pytest
import torch

import bf16_oracle as B
import mgunet
import mgunet_oracle as O
from mgunet import _lib
from mgunet.patch_graph import PatchGraphConstructor

pytestmark = pytest.mark.gpu


def sizes(case):
    cfg = B.CASES[case][0]
    cin, depth = cfg[0], cfg[3]
    if case == "f32d1":     # 2048 patches of 16 x 16 on one 32-channel N tile: launch_halo gives every workgroup two patches
        return {"ragged": (2, cin, 50, 70), "several_patches_per_workgroup": (8, cin, 256, 256)}
    out = {"small": (2, cin, 12, 20), "ragged": (3, cin, 37, 45) if case == "f32d2" else (2, cin, 50, 70), "whole": (1, cin, 64, 96)}
    if depth > 2:           # four halvings: no size below a patch leaves a bottleneck; 50 x 70 has 12 x 17, 6 x 8 and 3 x 4 below it
        del out["small"]
    return out


MATRIX = [(case, size) for case in B.CASES for size in sizes(case)]


def model(cfg, p, cuda):
    m = mgunet.UNet(*cfg, compute_dtype=torch.bfloat16)
    m.load_state_dict(p)
    return m.to(cuda).eval()


def profiled_forward(m, x, cuda):
    """One forward with the profiling records on: (outputs, {family: launches})."""
    ctx, L = m._context(cuda), _lib.lib()
    with torch.no_grad():
        m(x)                                        # (weights packed, workspace sized)
        torch.cuda.synchronize(cuda)
        _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
        out = m(x)
        torch.cuda.synchronize(cuda)
        ks = _lib.read_kernel_stats(ctx)
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return out, {k["name"]: k["launches"] for k in ks}


def assert_families(case, launched):
    cfg = B.CASES[case][0]
    want = B.family_launches(cfg)
    got = {n: c for n, c in launched.items() if n in B.FAMILY.values()}
    print(f"    [{case}] launched: {launched}")
    assert got == want, (case, got, want)
    for form, cin, cout in B.CASES[case][1]:        # what the case is there for is in the derived table
        assert (form, cin, cout) in B.layer_forms(cfg), (case, form, cin, cout)


@pytest.mark.parametrize("case,size", MATRIX)
def test_formula_weights_under_the_per_element_bar(cuda, case, size):
    cfg = B.CASES[case][0]
    depth = cfg[3]
    shape = sizes(case)[size]
    p = O.make_unet_params(*cfg, seed=21)
    x = torch.from_numpy(O.formula_normal(f"bf16layers/{case}/x", shape, seed=21))
    m = model(cfg, p, cuda)
    (lg, sk, ft), launched = profiled_forward(m, x.to(cuda), cuda)
    assert_families(case, launched)
    assert lg.dtype == torch.float32 and all(t.dtype == torch.bfloat16 for t in sk + ft)
    assert all(bool(torch.isfinite(t).all()) for t in [lg] + sk + ft)
    gsk = [t.double().cpu() for t in sk]
    gft = [t.double().cpu() for t in ft]
    first = B.first_fp32_weights(cfg[0], cfg[2])
    for name in B.segment_names(depth):
        got = (gsk if name.startswith("skip") else gft)[int(name[4:])]
        ref, floor = B.segment(p, depth, name, B.sources(depth, name, x, gsk, gft), first)
        B.check(got, ref, floor, f"{case} {size} {name}", deep=B.is_deep(depth, name))
    with torch.no_grad():
        head = torch.nn.functional.conv2d(ft[0].float().cpu(), p["decoder.final_conv.weight"], p["decoder.final_conv.bias"])
    d = float((lg.cpu() - head).abs().max())
    print(f"    [{case} {size}] logits <- feat0: max-abs {d:.2e} (fp32 head on the bf16 feature)")
    assert d <= 1e-4 * max(1.0, float(head.abs().max()))
    if shape[2] % 16 == 0 and shape[3] % 16 == 0:
        # node features requested from the forward == the stand-alone kernel on the returned bf16 feature == its float64 patch means
        pg = PatchGraphConstructor(16)
        ctx = m._context(cuda)
        with torch.no_grad():
            X0 = pg.patch_mean_features(ft[0])
            X1 = torch.full_like(X0, -7.0)
            _lib.check(_lib.lib().mgu_unet_request_patch_mean(ctx.handle, 16, X1.data_ptr()), ctx.handle)
            lg1, _, ft1 = m(x.to(cuda))
        assert torch.equal(ft1[0], ft[0])
        scale = max(1.0, float(X0.abs().max()))
        assert float((X1 - X0).abs().max()) <= 1e-6 * scale and float((lg1 - lg).abs().max()) <= 1e-5 * max(1.0, float(lg.abs().max()))
        Bn, C, H, W = gft[0].shape
        want = gft[0].reshape(Bn, C, H // 16, 16, W // 16, 16).mean(dim=(3, 5)).permute(0, 2, 3, 1).reshape(-1, C)
        # 256 bf16 values summed in fp32 in any order: (n - 1) * 2^-24 * mean|x| bounds the difference from the exact mean
        assert float((X0.double().cpu() - want).abs().max()) <= 255 * 2.0 ** -24 * float(gft[0].abs().max())


@pytest.mark.parametrize("case", list(B.CASES))
def test_exact_data_bit_for_bit(cuda, case):
    """Small-integer data on which the bf16 forward has exactly one right answer (bf16_oracle.exact_params): every index mapping of
    every kernel form -- pixel, channel, tap, k piece, swizzle, N tile, quadrant, pad row -- must come out bit for bit."""
    cfg = B.CASES[case][0]
    depth = cfg[3]
    m = None
    for seed in range(B.exact_seeds(cfg)):
        p = B.exact_params(cfg, seed)
        if m is None:
            m = model(cfg, p, cuda)
        else:
            m.load_state_dict(p)
        for size, shape in sizes(case).items():
            x = B.exact_input(shape, seed)
            lg, sk, ft = B.exact_reference(p, x, depth)
            for layout in ("nchw", "channels_last"):
                xg = x.to(cuda)
                if layout == "channels_last":
                    xg = xg.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                with torch.no_grad():
                    glg, gsk, gft = m(xg)
                    again = m(xg)
                tag = (case, seed, size, layout)
                for i in range(depth):
                    assert torch.equal(gsk[i].double().cpu(), sk[i]), tag + (f"skip{i}", _where(gsk[i], sk[i]))
                    assert torch.equal(gft[i].double().cpu(), ft[i]), tag + (f"feat{i}", _where(gft[i], ft[i]))
                assert torch.equal(glg.double().cpu(), lg), tag + ("logits", _where(glg, lg))
                for a, b in zip([glg] + gsk + gft, [again[0]] + again[1] + again[2]):
                    assert torch.equal(a, b), tag + ("a second call returns other bytes",)


def _where(got, ref):
    """Where a failing tensor differs: count, channel range and the first pixels (patch position = y % 16, x % 16)."""
    bad = (got.double().cpu() != ref).nonzero()
    if bad.numel() == 0:
        return "equal"
    return (f"{bad.shape[0]} of {ref.numel()} differ; channels {int(bad[:, 1].min())}..{int(bad[:, 1].max())}, rows "
            f"{int(bad[:, 2].min())}..{int(bad[:, 2].max())}, columns {int(bad[:, 3].min())}..{int(bad[:, 3].max())}; first {bad[:4].tolist()}")
