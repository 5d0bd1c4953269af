"""The assembly Winograd kernels (csrc/asm/gen_wino_cp.py) form the tile-column inner sum the two components of a pair share once,
in the jj = 0 step, and the jj = 1 step of the same mi takes it from the raw registers.  Every value still comes from the same IEEE
instructions on the same operands, so the kernels stay bitwise equal to the C++ kernels they replace (MGU_WINO_ASM 1 vs 0).
test_gpu_wino_asm.py covers the inference epilogue; this file adds the paths it does not take:
  * NULL scale and shift (the training dgrad path: the kernels' 1 / 0 defaults) on the wide kernel and on both narrow kernels;
  * workgroups that walk an odd number of patches (the shared sums cross the patch epilogue with the next patch's first reads),
    across interior / edge patches and a last workgroup with a shorter walk."""
import pytest
import torch
import torch.nn.functional as F

import mgunet_oracle as O
from mgunet import _lib
from mgunet import gat as G

pytestmark = pytest.mark.gpu


def _conv(cuda, xin, wd, sc, sh, Cout, relu, ld, off):
    B, H, W, Cin = xin.shape
    out = torch.full((B, H, W, ld), -7.0, device=cuda)
    ctx = G._context(cuda)
    rc = _lib.lib().mgu_conv2d_nhwc(ctx.handle, xin.data_ptr(), B, H, W, Cin, wd.data_ptr(), None,
                                    None if sc is None else sc.data_ptr(), None if sh is None else sh.data_ptr(),
                                    Cout, 3, relu, out.data_ptr(), ld, off, _lib.current_stream_ptr(cuda))
    _lib.check(rc, ctx.handle)
    torch.cuda.synchronize()
    return out


def _both_arms(cuda, monkeypatch, B, H, W, Cin, Cout, relu, affine):
    x = torch.from_numpy(O.formula_normal("wsc/x", (B, Cin, H, W), seed=H + Cin + B))
    w = torch.from_numpy(O.formula_uniform("wsc/w", (Cout, Cin, 3, 3), -0.2, 0.2, seed=W + Cout))
    sc = sh = None
    if affine:
        sc = torch.from_numpy(O.formula_uniform("wsc/sc", (Cout,), 0.5, 1.5, seed=3)).to(cuda)
        sh = torch.from_numpy(O.formula_uniform("wsc/sh", (Cout,), -0.5, 0.5, seed=4)).to(cuda)
    xin, wd = x.permute(0, 2, 3, 1).contiguous().to(cuda), w.contiguous().to(cuda)
    ld, off = Cout + 8, 4
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("MGU_WINO_ASM", flag)
        G._CTX.clear()
        outs.append(_conv(cuda, xin, wd, sc, sh, Cout, relu, ld, off))
    monkeypatch.delenv("MGU_WINO_ASM")
    G._CTX.clear()
    cpp, asm = outs
    assert torch.all(asm[..., :off] == -7.0) and torch.all(asm[..., off + Cout:] == -7.0)
    if not torch.equal(asm, cpp):
        bad = (asm != cpp).nonzero()
        raise AssertionError(f"{bad.shape[0]} of {asm.numel()} values differ; first at (b, y, x, c) = {bad[0].tolist()}: "
                             f"{asm[tuple(bad[0])].item()!r} vs {cpp[tuple(bad[0])].item()!r}")
    ref = F.conv2d(x, w, None, padding=1)
    if affine:
        ref = ref * sc.cpu().view(1, -1, 1, 1) + sh.cpu().view(1, -1, 1, 1)
    ref = F.relu(ref) if relu else ref
    got = asm[..., off:off + Cout].permute(0, 3, 1, 2).cpu()
    assert float((got - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("B,H,W,Cin,Cout", [
    (1, 128, 128, 64, 64),    # wide kernel
    (1, 128, 128, 32, 32),    # narrow, two chunks (mgu_wino_cp1r2_gfx950)
    (1, 128, 128, 64, 32),    # narrow, four chunks (mgu_wino_cp1r4_gfx950)
])
@pytest.mark.parametrize("relu", [0, 1])
def test_null_scale_and_shift_bit_for_bit(cuda, monkeypatch, B, H, W, Cin, Cout, relu):
    _both_arms(cuda, monkeypatch, B, H, W, Cin, Cout, relu, affine=False)


@pytest.mark.parametrize("Cin,Cout", [(32, 64), (32, 32), (64, 32)])
def test_odd_patch_walk_across_edges_bit_for_bit(cuda, monkeypatch, Cin, Cout):
    # 800 x 320: 100 x 10 patches -> 3 patches per workgroup (1000 / 256), 334 workgroups, the last one walks a single patch;
    # a walk of three runs from interior patches into the edge patches of a row and on into the next row
    _both_arms(cuda, monkeypatch, 1, 800, 320, Cin, Cout, 1, affine=True)
