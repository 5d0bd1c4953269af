"""The hand-scheduled assembly form of the fp32 ConvTranspose2d(2, 2) forward kernel (csrc/asm/gen_convt_x3.py, mgu_convt_x3_gfx950)
against the C++ kernel it replaces (convt2x2_x3_kernel<0, 2>, csrc/convt_x3.hip): the same arithmetic in the same order, so the two
must be EQUAL BIT FOR BIT.  MGU_CONVT_ASM is read by mgu_create: each arm runs in a context of its own.  The profiling label is the
same for both, so mgu_convt_asm_launches tells which kernel a launch took."""
import pytest
import torch

import mgunet_oracle as O
from mgunet import _lib
from mgunet import gat as G

pytestmark = pytest.mark.gpu


def _convt(cuda, monkeypatch, flag, xin, wd, bias, Cout):
    """-> (the whole concat buffer, assembly launches of the context)"""
    B, H, W, Cin = xin.shape
    if flag is None:
        monkeypatch.delenv("MGU_CONVT_ASM", raising=False)
    else:
        monkeypatch.setenv("MGU_CONVT_ASM", flag)
    G._CTX.clear()
    ctx = G._context(cuda)
    out = torch.full((B, 2 * H, 2 * W, 2 * Cout), -7.0, device=cuda)
    rc = _lib.lib().mgu_conv_transpose2x2_nhwc(ctx.handle, xin.data_ptr(), B, H, W, Cin, wd.data_ptr(), bias.data_ptr(), Cout,
                                               out.data_ptr(), 2 * Cout, Cout, _lib.current_stream_ptr(cuda))
    _lib.check(rc, ctx.handle)
    torch.cuda.synchronize()
    n = int(_lib.lib().mgu_convt_asm_launches(ctx.handle))
    monkeypatch.delenv("MGU_CONVT_ASM", raising=False)
    G._CTX.clear()
    return out, n


# (B, H, W, Cin, Cout), written at coff = Cout into a 2 Cout pitch; asm: the shape is one the assembly kernel takes
SHAPES = [
    (1, 8, 16, 32, 32, True),      # one pixel tile, one column tile, a single K = 32 step: prologue and epilogue only, odd step count
    (1, 8, 16, 64, 64, True),      # two steps, two column tiles
    (1, 8, 16, 96, 32, True),      # three steps: the loop's odd tail
    (2, 8, 32, 64, 32, True),      # tiles that cross rows and the image boundary
    (1, 16, 16, 128, 128, True),   # four column tiles: the same pixel rows re-read under the XCD remap
    (1, 6, 8, 32, 32, False),      # M = 48: falls back to the C++ kernel
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,asm", SHAPES)
def test_assembly_kernel_equals_cpp_kernel_bit_for_bit(cuda, monkeypatch, B, H, W, Cin, Cout, asm):
    x = torch.from_numpy(O.formula_normal("cta/x", (B, H, W, Cin), seed=H + Cin)).to(cuda)
    w = torch.from_numpy(O.formula_uniform("cta/w", (Cin, Cout, 2, 2), -0.2, 0.2, seed=W + Cout)).to(cuda)
    b = torch.from_numpy(O.formula_uniform("cta/b", (Cout,), -0.5, 0.5, seed=3)).to(cuda)
    cpp, n_cpp = _convt(cuda, monkeypatch, "0", x, w, b, Cout)
    got, n_asm = _convt(cuda, monkeypatch, None, x, w, b, Cout)
    assert n_cpp == 0
    assert n_asm == (1 if asm else 0)          # the only ConvTranspose launch of the context
    assert torch.all(got[..., :Cout] == -7.0)  # the skip half of the concat buffer
    if not torch.equal(got, cpp):
        bad = (got != cpp).nonzero()
        raise AssertionError(f"{bad.shape[0]} of {got.numel()} values differ; first at (b, y, x, c) = {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])].item()!r} vs {cpp[tuple(bad[0])].item()!r}")
    # and the C++ arm is the operator (three-piece products: fp32 accuracy)
    ref = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), stride=2).permute(0, 2, 3, 1)
    assert float((cpp[..., Cout:].double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("shape", [(1, 64, 256), (2, 128, 128)])
def test_whole_network_equal_on_both_kernels(cuda, monkeypatch, shape):
    """UNet(3, 2, 32, 4): logits, skips and decoder features equal between the two contexts; the count tells which ConvTranspose
    layers took the assembly kernel -- those whose image group has M = n H W % 128 == 0 on the layer's input grid."""
    import mgunet
    cfg = (3, 2, 32, 4)
    B, H, W = shape
    p = O.make_unet_params(*cfg, seed=11)
    x = torch.from_numpy(O.formula_normal("cta/img", (B, 3, H, W), seed=3)).to(cuda)
    groups = [B] if B < 2 else [(B + 1) // 2, B - (B + 1) // 2]                      # the eval forward walks two half batches
    want = sum(1 for n in groups for l in range(1, 5) if n * (H >> l) * (W >> l) % 128 == 0)
    assert 0 < want < 4 * len(groups)                                                # both kernels appear in this forward
    outs, counts = [], []
    for flag in ("0", None):
        if flag is None:
            monkeypatch.delenv("MGU_CONVT_ASM", raising=False)
        else:
            monkeypatch.setenv("MGU_CONVT_ASM", flag)
        unet = mgunet.UNet(*cfg)
        unet.load_state_dict(p)
        unet = unet.to(cuda).eval()
        lg, sk, ft = unet(x)
        torch.cuda.synchronize()
        outs.append([lg.clone()] + [t.clone() for t in sk] + [t.clone() for t in ft])
        counts.append(int(_lib.lib().mgu_convt_asm_launches(unet._context(cuda).handle)))
        del unet
    monkeypatch.delenv("MGU_CONVT_ASM", raising=False)
    assert counts == [0, want]
    for a, b in zip(*outs):
        assert torch.equal(a, b)
