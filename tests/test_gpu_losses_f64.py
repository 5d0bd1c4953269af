"""The auxiliary-loss kernels of csrc/losses.hip (TV, dice, feature consistency, elliptical shape: values and gradients) and
FeatureFusion's two kernels of csrc/imageops.hip (bilinear resize, region-map gather) against float64, at the shapes, layouts and
edges where they take another path: every template form and lane trip, every workgroup cap, strided and non-dense views, the
accumulate / device-scale path of the dice backward, exact zeros, exact ties, untouched neighbours.

Cases, references and bars are tests/losses_cases.py (bar = 4 * cond + 2^-22 with cond the fp32 oracle's own deviation from
float64 on the case, never above the fixture tests' bar; the shape loss 5e-7; gathers, zero gradients and untouched channels
exact).  Every element of every gradient is compared.  NOTES.md ("Auxiliary losses and FeatureFusion: float64 bars") carries cond,
the bar and the measured error of every line these tests print under -s."""
import numpy as np
import pytest
import torch

import losses_cases as LC
import mgunet
from mgunet import _lib

pytestmark = pytest.mark.gpu

ids = lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


def leaf(view):
    return view.detach().requires_grad_(True)


# ---- total variation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LC.TV_SHAPES, ids=ids)
def test_tv_value_and_gradient(cuda, shape):
    ref = LC.tv_reference(shape)
    tv = mgunet.TVLoss(LC.TV_WEIGHT)
    x = LC.tv_input(shape).to(cuda)
    base = None
    for name in LC.tv_layouts(shape):
        xl = leaf(LC.TV_LAYOUTS[name](x))
        v = tv(xl)
        LC.tv_post(False)(v).backward()                             # an upstream factor
        what = f"tv {shape} {name}"
        ref.check("value", v.detach(), LC.CAP["value"], what)
        ref.check("dx", xl.grad, LC.CAP["tv"], what)
        assert tuple(xl.grad.shape) == tuple(shape)
        if base is None:
            base = xl.grad.clone()
        assert LC.err_of("dx", xl.grad, base) <= ref.bar("dx", LC.CAP["tv"]), what   # the same gradient whatever the storage
    if shape == LC.TV_CHAINED:                                      # grad_output = TV_UP + v: a device scalar that is no constant
        chained = LC.tv_reference(shape, True)
        for name in ("nhwc", "crop"):
            xl = leaf(LC.TV_LAYOUTS[name](x))
            v = tv(xl)
            LC.tv_post(True)(v).backward()
            chained.check("value", v.detach(), LC.CAP["value"], f"tv {shape} {name} chained")
            chained.check("dx", xl.grad, LC.CAP["tv"], f"tv {shape} {name} chained")


@pytest.mark.parametrize("shape", [(2, 3, 1, 9), (2, 3, 9, 1), (1, 1, 1, 1)], ids=ids)
def test_tv_one_row_or_column_raises(cuda, shape):
    """The reference divides by (H - 1) W or H (W - 1) = 0 there; the library refuses, and launches nothing."""
    B, C, H, W = shape
    x = torch.ones(shape, device=cuda)
    with pytest.raises(ValueError, match="H, W >= 2"):
        mgunet.TVLoss()(x)
    out = torch.full((), -5.0, device=cuda)
    dx = torch.full(shape, -5.0, device=cuda)
    one = torch.ones((), device=cuda)
    with pytest.raises(ValueError, match="H, W >= 2"):
        _lib.call("mgu_tv_loss", cuda, x, B, C, H, W, *x.stride(), 1.0, out)
    with pytest.raises(ValueError, match="H, W >= 2"):
        _lib.call("mgu_tv_loss_backward", cuda, x, B, C, H, W, *x.stride(), 1.0, 1.0, one, dx, *dx.stride())
    assert float(out) == -5.0 and bool((dx == -5.0).all())


# ---- dice ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(LC.DICE_CASES))
def test_dice_value_and_gradient(cuda, tag):
    B, C, H, W, _, _ = LC.DICE_CASES[tag]
    lg, y, smooth = LC.dice_inputs(tag)
    ref = LC.dice_reference(tag)
    lgd, yd = lg.to(cuda), y.to(cuda)
    for name, lay in LC.DICE_LAYOUTS.items():
        l = leaf(lay(lgd))
        v = mgunet.dice_loss(l, yd, smooth)
        v.backward()
        what = f"dice {tag} {name}"
        ref.check("value", v.detach(), LC.CAP["value"], what)
        ref.check("dlogits", l.grad, LC.CAP["dice"], what)
        assert tuple(l.grad.shape) == (B, C, H, W) and bool(torch.isfinite(l.grad).all())
        if C == 1:                                                  # softmax over one class is 1: nothing reaches the logits
            assert float(l.grad.abs().max()) == 0.0 and float(v.detach()) == 0.0
    mgunet.losses.check_labels(cuda)


def test_dice_nine_classes_raises(cuda):
    lg = torch.zeros(1, 9, 4, 4, device=cuda, requires_grad=True)
    with pytest.raises(ValueError, match="num_classes <= 8"):
        mgunet.dice_loss(lg, torch.zeros(1, 4, 4, dtype=torch.int64, device=cuda))


@pytest.mark.parametrize("tag", LC.DICE_RAW)
def test_dice_backward_accumulate_raw_abi(cuda, tag):
    """mgu_dice_loss_backward as Trainer(loss="ce+dice") calls it: adding into a destination of pitch 8, grad_scale together with
    grad_scale_dev, the loss written by the same call.  C = 3 runs the <4> kernels, C = 6 the <8> kernels."""
    B, C, H, W, _, _ = LC.DICE_CASES[tag]
    HW, pitch = H * W, LC.DICE_RAW_PITCH
    lg, y, smooth = LC.dice_inputs(tag)
    lgd, yd = lg.to(cuda).contiguous(), y.to(cuda).contiguous()
    pre = LC.dice_raw_prefill(tag).to(cuda)
    dst = pre.clone()
    assert tuple(dst.shape) == (B * HW, pitch) and dst.is_contiguous()
    scale_dev = torch.tensor([LC.DICE_RAW_SCALE_DEV], device=cuda, dtype=torch.float32)
    loss = torch.full((), -5.0, device=cuda, dtype=torch.float32)
    _lib.call("mgu_dice_loss_backward", cuda, lgd, yd, B, HW, C, C * HW, HW, 1, smooth, LC.DICE_RAW_SCALE, scale_dev, dst, HW * pitch, 1,
              pitch, 1, loss)
    LC.dice_raw_reference(tag).check("acc", dst[:, :C], LC.CAP["dice"], f"dice accumulate {tag}")
    assert torch.equal(dst[:, C:], pre[:, C:])                      # channels [C, 8) keep their bytes
    LC.dice_reference(tag).check("value", loss, LC.CAP["value"], f"dice accumulate {tag}")
    mgunet.losses.check_labels(cuda)


# ---- feature consistency ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(LC.FEATCONS_CASES))
def test_feature_consistency_value_and_gradients(cuda, tag):
    B, N, D, mrule, _, coin, _ = LC.FEATCONS_CASES[tag]
    fu, fg, y, margin, needs = LC.featcons_inputs(tag)
    ref = LC.featcons_reference(tag)
    a, b = fu.to(cuda).requires_grad_(needs[0]), fg.to(cuda).requires_grad_(needs[1])
    v = mgunet.FeatureConsistencyLoss(margin=margin)(a, b, y.to(cuda))
    (LC.FEATCONS_UP * v).backward()
    what = f"feature consistency {tag}"
    ref.check("value", v.detach(), LC.CAP["value"], what)
    for t, need, name in ((a, needs[0], "dfu"), (b, needs[1], "dfg")):
        if not need:
            assert t.grad is None
            continue
        ref.check(name, t.grad, LC.CAP["featcons"], what)
        assert tuple(t.grad.shape) == (B, N, D) and bool(torch.isfinite(t.grad).all())
        if coin is not None:                                        # dist = 1e-4 is a divisor; 0 * k stays 0
            assert float(t.grad[0, 0].abs().max()) == 0.0
        if mrule == "below":                                        # no hinge anywhere: rows with y = 0 get no gradient
            assert float(t.grad[(y == 0).to(cuda)].abs().max()) == 0.0


# ---- elliptical shape ---------------------------------------------------------------------------------------------------------------
def shape_check(what, got, ref):
    err = abs(float(got) - ref) / max(1.0, abs(ref))
    print(f"| {what} | value | - | {LC.SHAPE_BAR:.1e} | {err:.1e} |")
    assert err <= LC.SHAPE_BAR, (what, float(got), ref)


def test_shape_loss_masks_seventy_objects(cuda):
    """70 objects in one call: objects 64 .. 69 are the second workgroup of shape_params_kernel, and hold both sides of the
    10-pixel threshold, the one-pixel-wide objects and the empty mask."""
    masks = LC.shape_masks()
    dev = [torch.from_numpy(m).to(cuda) for m in masks]
    got = mgunet.EllipticalShapeLoss(epsilon=LC.SHAPE_EPS)(None, object_masks_list=[dev[:33], dev[33:]])
    shape_check("shape masks 70 x 24 x 24", got, LC.shape_reference(masks))
    # the second workgroup alone, and a call whose every object is skipped
    got = mgunet.EllipticalShapeLoss(epsilon=LC.SHAPE_EPS)(None, object_masks_list=[dev[64:]])
    shape_check("shape masks objects 64 .. 69", got, LC.shape_reference(masks[64:]))
    skipped = [dev[-1], dev[64]]
    assert float(mgunet.EllipticalShapeLoss(epsilon=LC.SHAPE_EPS)(None, object_masks_list=[skipped])) == 0.0


def test_shape_loss_masks_over_the_workgroup_cap(cuda):
    big = LC.shape_big_masks()
    got = mgunet.EllipticalShapeLoss(epsilon=LC.SHAPE_EPS)(None, object_masks_list=[[torch.from_numpy(m).to(cuda) for m in big]])
    shape_check("shape masks 2 x 520 x 520", got, LC.shape_reference(big))


@pytest.mark.parametrize("store", ["nchw", "nhwc"])
@pytest.mark.parametrize("C", LC.PROBS_CLASSES)
def test_shape_loss_probabilities(cuda, C, store):
    p = LC.probs_input(C).to(cuda)
    p = LC.lay_nhwc(p) if store == "nhwc" else p
    assert (p.stride(1) == 1) == (store == "nhwc")
    got = mgunet.EllipticalShapeLoss(epsilon=LC.SHAPE_EPS)(p)
    shape_check(f"shape probabilities C = {C} {store}", got, LC.probs_case_reference(C))


# ---- FeatureFusion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", LC.RESIZE_CHANNELS)
@pytest.mark.parametrize("src,dst", LC.RESIZE_SIZES, ids=ids)
def test_feature_fusion_resize(cuda, src, dst, C):
    B, (h, w), (Ho, Wo) = LC.RESIZE_B, src, dst
    ref = LC.resize_reference(src, dst, C)
    x = LC.resize_input(src, C).to(cuda)
    what = f"resize {src} -> {dst} C = {C}"
    same = torch.from_numpy(LC.O.formula_normal("lcase/resize/g", (B, 4, Ho, Wo), seed=3)).to(cuda)
    fused = mgunet.FeatureFusion([C], 4)([x], same, target_spatial_size=dst)
    assert tuple(fused.shape) == (B, C + 4, Ho, Wo)
    ref.check("map", fused[:, :C], LC.CAP["resize"], what)
    assert torch.equal(fused[:, C:], same)
    # the binding itself, into channels [8, 8 + C) of a 48-wide sentinel-filled map: nothing else may change
    out = torch.full((B, Ho, Wo, LC.RESIZE_LD), LC.SENTINEL, device=cuda)
    _lib.call("mgu_resize_bilinear_nhwc", cuda, x.permute(0, 2, 3, 1).contiguous(), C, B, h, w, C, out, LC.RESIZE_LD, LC.RESIZE_OFF, Ho, Wo)
    lo, hi = LC.RESIZE_OFF, LC.RESIZE_OFF + C
    ref.check("map", out[..., lo:hi].permute(0, 3, 1, 2), LC.CAP["resize"], what + " direct")
    assert bool((out[..., :lo] == LC.SENTINEL).all()) and bool((out[..., hi:] == LC.SENTINEL).all())
    assert torch.equal(out[..., lo:hi].permute(0, 3, 1, 2), fused[:, :C])


@pytest.mark.parametrize("D", LC.GATHER_DIMS)
def test_feature_fusion_region_map_gather(cuda, D):
    B, H, W, R = LC.GATHER_B, LC.GATHER_H, LC.GATHER_W, LC.GATHER_R
    table, ids_ = LC.gather_inputs(D)
    ref = LC.gather_reference(table, ids_)
    out = torch.full((B, H, W, LC.GATHER_LD), LC.SENTINEL, device=cuda)
    _lib.call("mgu_region_map_gather_nhwc", cuda, table.to(cuda), R, D, ids_.to(cuda), B * H * W, out, LC.GATHER_LD, LC.GATHER_OFF)
    lo, hi = LC.GATHER_OFF, LC.GATHER_OFF + D
    assert torch.equal(out[..., lo:hi].cpu(), ref)                  # valid rows the table's bytes, invalid rows exactly 0
    assert bool((out[..., :lo] == LC.SENTINEL).all()) and bool((out[..., hi:] == LC.SENTINEL).all())
    fu = torch.from_numpy(LC.O.formula_normal("lcase/gather/u", (B, 4, H, W), seed=D)).to(cuda)
    fused = mgunet.FeatureFusion([4], D)([fu], table.to(cuda), region_to_pixel_map=ids_.to(cuda))
    assert torch.equal(fused[:, :4], fu) and torch.equal(fused[:, 4:].permute(0, 2, 3, 1).cpu(), ref)
