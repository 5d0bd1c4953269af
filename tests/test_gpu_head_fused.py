"""The head-fused finishing pass of the convolution that writes decoder feature 0 (mgu_wino_cp1r2h_gfx950, csrc/asm/gen_wino_cp.py,
and its C++ twin wino3x3_cp_kernel<1, head>, csrc/wino_f32.hip): with a pending patch-mean request at the graph's 16-pixel patch
the final 1x1 conv (unet_decoder.py:117,143) and the patch sums ride in that launch, and patch_mean_kernel's second pass over the
feature map falls away.  MGU_HEAD_FUSED=0 restores the two-kernel path; the switch is read when a model's context is created, so
every arm below is a model (and a context) of its own.

What must hold:
  * every feature tensor is EQUAL BIT FOR BIT between the two paths (the main loop, the share exchange and the feature stores of
    the fused kernel are the plain kernel's);
  * logits and patch means are fp32 evaluations of the same 32-term dot product and 256-term mean in another order, so they are
    compared, both paths, with a float64 recomputation from the HIP path's own decoder feature 0: the fused path's worst deviation
    may be at most TWICE the stand-alone kernel's on the same inputs (the factor is room for a different, equally valid order);
  * the assembly kernel and its C++ twin agree bit for bit on features, logits and patch means;
  * two fused forwards agree bit for bit (plain stores and a fixed-order combine: no atomics);
  * ragged sizes, other patch sizes, bf16 storage and training forwards stay on the stand-alone kernel (profiling records)."""
import pytest
import torch

import mgunet
import mgunet_oracle as O
from mgunet import _lib

pytestmark = pytest.mark.gpu

CFG = (3, 2, 32, 4)
# the class count selects hand-written branches of the fused kernels (fma / fold chains per class, a store variant per count): every
# count the pick admits runs at a small shape, the headline count at all shapes
SHAPES_NCLS = [((8, 512, 512), 2), ((1, 64, 64), 1), ((1, 64, 64), 2), ((1, 64, 64), 3), ((1, 64, 64), 4), ((3, 48, 96), 2), ((3, 48, 96), 3)]
FUSED, COMBINE, STANDALONE = "mgu_wino_cp1r2h_gfx950", "patch_sum_combine_kernel", "patch_mean_kernel"
# shapes: the headline step and two smaller eligible ones (H % 16 == 0, W % 32 == 0)


def _forward(cuda, monkeypatch, env, shape, patch=16, dtype=torch.float32, train=False, runs=1, ncls=2):
    """-> ([(logits, skips, feats, patch means)] per run, profiled kernel names of the last run, the model) of a fresh model under `env`"""
    for k in ("MGU_HEAD_FUSED", "MGU_WINO_ASM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, H, W = shape
    cfg = (CFG[0], ncls) + CFG[2:]
    m = mgunet.UNet(*cfg, compute_dtype=dtype)
    m.load_state_dict(O.make_unet_params(*cfg, seed=3))
    m = m.to(cuda)
    m = m.train() if train else m.eval()
    x = torch.from_numpy(O.formula_normal("head_fused/x", (B, 3, H, W), seed=H + W)).to(cuda)
    ctx, L = m._context(cuda), _lib.lib()
    nodes = B * ((H + patch - 1) // patch) * ((W + patch - 1) // patch)
    outs = []
    for r in range(runs):
        pm = torch.full((nodes, CFG[2]), float("nan"), device=cuda)
        if r == runs - 1:
            _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
        _lib.call("mgu_unet_request_patch_mean", cuda, patch, pm, ctx=ctx)
        with torch.no_grad():
            lg, sk, ft = m(x)
        torch.cuda.synchronize(cuda)
        outs.append((lg.clone(), [t.clone() for t in sk], [t.clone() for t in ft], pm))
    names = [k["name"] for k in _lib.read_kernel_stats(ctx)]
    _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return outs, names, m


def _deviation(m, lg, feat0, pm, patch=16):
    """worst |logit| and |patch mean| deviation from the float64 evaluation on the path's own decoder feature 0"""
    f = feat0.double()
    sd = m.state_dict()
    w = sd["decoder.final_conv.weight"].double()[:, :, 0, 0]
    b = sd["decoder.final_conv.bias"].double()
    ref_lg = torch.einsum("bchw,kc->bkhw", f, w) + b.view(1, -1, 1, 1)
    B, C, H, W = f.shape
    ref_pm = f.view(B, C, H // patch, patch, W // patch, patch).mean(dim=(3, 5)).permute(0, 2, 3, 1).reshape(-1, C)
    return float((lg.double() - ref_lg).abs().max()), float((pm.double() - ref_pm).abs().max())


@pytest.mark.parametrize("shape,ncls", SHAPES_NCLS)
def test_features_equal_and_head_within_twice_the_standalone_deviation(cuda, monkeypatch, shape, ncls):
    """Measured on MI355X (worst |deviation| from float64, stand-alone -> fused):
      8 x 512 x 512: logits 1.12e-06 -> 8.64e-07, patch means 9.09e-07 -> 5.64e-07
      1 x  64 x  64: logits 5.43e-07 -> 4.32e-07, patch means 3.52e-07 -> 2.33e-07
      3 x  48 x  96: logits 7.32e-07 -> 5.40e-07, patch means 3.62e-07 -> 3.23e-07"""
    (a,), na, ma = _forward(cuda, monkeypatch, {"MGU_HEAD_FUSED": "0"}, shape, ncls=ncls)
    (f,), nf, mf = _forward(cuda, monkeypatch, {"MGU_HEAD_FUSED": "1"}, shape, ncls=ncls)
    assert any(STANDALONE in n for n in na) and not any(FUSED in n or COMBINE in n for n in na), na
    assert any(FUSED in n for n in nf) and any(COMBINE in n for n in nf) and not any(STANDALONE in n for n in nf), nf
    for i, (u, v) in enumerate(zip(a[1] + a[2], f[1] + f[2])):   # skips, decoder features
        assert torch.equal(u, v), f"exposed tensor {i} differs between the two paths"
    sa_lg, sa_pm = _deviation(ma, a[0], a[2][0], a[3])
    fu_lg, fu_pm = _deviation(mf, f[0], f[2][0], f[3])
    print(f"\n{shape} ncls {ncls}: |logit - f64| stand-alone {sa_lg:.3e} fused {fu_lg:.3e}; |patch mean - f64| stand-alone {sa_pm:.3e} fused {fu_pm:.3e}")
    assert torch.isfinite(f[3]).all() and torch.isfinite(f[0]).all()
    assert fu_lg <= 2 * sa_lg, (fu_lg, sa_lg)
    assert fu_pm <= 2 * sa_pm, (fu_pm, sa_pm)


@pytest.mark.parametrize("shape,ncls", SHAPES_NCLS)
def test_assembly_kernel_equals_its_cpp_twin(cuda, monkeypatch, shape, ncls):
    (a,), na, _ = _forward(cuda, monkeypatch, {"MGU_HEAD_FUSED": "1"}, shape, ncls=ncls)
    (c,), nc, _ = _forward(cuda, monkeypatch, {"MGU_HEAD_FUSED": "1", "MGU_WINO_ASM": "0"}, shape, ncls=ncls)
    assert any(FUSED in n for n in na), na
    assert any("wino3x3_cp_kernel<1, head>" in n for n in nc) and not any(STANDALONE in n or "gfx950" in n for n in nc), nc
    assert torch.equal(a[0], c[0]), "logits"
    assert torch.equal(a[3], c[3]), "patch means"
    for i, (u, v) in enumerate(zip(a[1] + a[2], c[1] + c[2])):
        assert torch.equal(u, v), f"exposed tensor {i}"


@pytest.mark.parametrize("shape,ncls", SHAPES_NCLS)
def test_fused_forward_is_repeatable(cuda, monkeypatch, shape, ncls):
    (r0, r1), names, _ = _forward(cuda, monkeypatch, {}, shape, runs=2, ncls=ncls)   # the default IS the fused route
    assert any(FUSED in n for n in names), names
    assert torch.equal(r0[0], r1[0]) and torch.equal(r0[3], r1[3])
    for u, v in zip(r0[1] + r0[2], r1[1] + r1[2]):
        assert torch.equal(u, v)


@pytest.mark.parametrize("case,shape,kw", [
    ("ragged", (1, 48, 80), {}),                                  # W % 32 != 0
    ("ragged rows", (1, 40, 64), {}),                             # H % 16 != 0 (the graph pads its last patch row)
    ("patch 8", (1, 64, 64), {"patch": 8}),
    ("bf16 storage", (1, 64, 64), {"dtype": torch.bfloat16}),
    ("training forward", (2, 64, 64), {"train": True}),
    ("five classes", (1, 64, 64), {"ncls": 5}),
])
def test_everything_else_stays_on_the_standalone_kernel(cuda, monkeypatch, case, shape, kw):
    (o,), names, _ = _forward(cuda, monkeypatch, {}, shape, **kw)
    assert any(STANDALONE in n for n in names), (case, names)
    assert not any(FUSED in n or COMBINE in n or "head>" in n for n in names), (case, names)
    assert torch.isfinite(o[3]).all(), case
