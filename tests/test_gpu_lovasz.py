"""The Lovasz-Softmax kernels (csrc/lovasz.hip) on the GPU: the segmented radix sort against the tie rule (exact), value and gradient
against float64 with the device's own ranks pinned, at the segment sizes around the workgroup tile, at the key's edges (errors of
exactly 0 and 1, one giant tie, errors that differ in the lowest / the highest digit only), every class count form, every storage
layout, the raw ABI as the trainer calls it, bad labels and limits, bitwise reproducibility, and Trainer(loss="ce+lovasz").

Cases, reference and bars: tests/lovasz_cases.py (bar = 4 * cond + 2^-22, cond = the same code in fp32 under the same pinned ranks;
caps 2e-6 for the value, 5e-6 for gradients and for the device's errors).  NOTES.md ("Lovasz-Softmax: float64 bars") carries the
lines these tests print under -s."""
import numpy as np
import pytest
import torch

import lovasz_cases as LV
import mgunet
import mgunet_oracle as O
from mgunet import _lib
from mgunet.losses import _lovasz_debug

pytestmark = pytest.mark.gpu

T = 4096            # mgu_lovasz_tile() of the library this suite was written against; test_tile_size holds the two together
ALL_TAGS = list(LV.cases(T))


def leaf(view):
    return view.detach().requires_grad_(True)


def run_case(cuda, tag, layout="nchw"):
    """(value, gradient, errors, ranks) of the device for the case, the last two on the host"""
    lg, y, classes, per_image = LV.inputs(tag, T)
    yd = y.to(cuda)
    l = leaf(LV.LAYOUTS[layout](lg.to(cuda)))
    v = mgunet.lovasz_softmax(l, yd, classes=classes, per_image=per_image)
    v.backward()
    dv, errors, ranks = _lovasz_debug(l.detach(), yd, classes=classes, per_image=per_image)
    assert torch.equal(dv, v.detach())                              # the hooks change nothing
    return v.detach(), l.grad, errors.cpu(), ranks.cpu()


def test_tile_size(cuda):
    assert int(_lib.lib().mgu_lovasz_tile()) == T


@pytest.mark.parametrize("tag", ALL_TAGS)
def test_ranks_value_and_gradient(cuda, tag):
    B, C, H, W, kind, classes, per_image = LV.cases(T)[tag]
    lg, y, _, _ = LV.inputs(tag, T)
    v, grad, errors, ranks = run_case(cuda, tag)
    mgunet.losses.check_labels(cuda)
    what = f"lovasz {tag} ({B}x{C}x{H}x{W} {classes}{' per image' if per_image else ''})"
    # 1. the sort: exact against the device's own errors; the errors against the float64 softmax
    assert tuple(errors.shape) == tuple(ranks.shape) == (C, B, H, W)
    ties = LV.check_ranks(errors.numpy(), ranks.numpy(), y.numpy(), per_image)
    LV.errors_reference(tag, T).check("errors", errors, LV.CAP["errors"], what)
    # 2. value and every element of the gradient with those ranks pinned; the value also against the reference's own sort
    ref = LV.reference(tag, T, ranks.numpy())
    ref.check("value", v, LV.CAP["value"], what)
    ref.check("grad", grad, LV.CAP["grad"], what)
    free = LV.reference(tag, T)
    assert LV.err_of("value", v, free.r64["value"]) <= ref.bar("value", LV.CAP["value"]), what
    assert tuple(grad.shape) == (B, C, H, W) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(v))
    if bool((y == LV.IGNORE).any()):                                # an ignored pixel gets exactly no gradient
        assert float(grad.permute(0, 2, 3, 1)[(y == LV.IGNORE).to(cuda)].abs().max()) == 0.0
    # 3. what the case is there for
    bits = errors.numpy().view(np.uint32)
    if kind == "saturated":       # errors exactly 0.0 / 1.0 (the 30-bit boundary key); the value is 1 - IoU of the arg-max map in fp32
        assert set(np.unique(bits)) == {0, 0x3F800000}
        pred = lg.argmax(1)
        ious = [1.0 - float(((pred == c) & (y == c)).sum()) / float(((pred == c) | (y == c)).sum()) for c in range(C) if bool((y == c).any())]
        assert float(v) == float(np.float32(sum(ious) / len(ious)))
    if kind == "equal":           # one tie spanning the segment: ranks are pixel order
        assert len(np.unique(bits[0])) <= 2 and ties > 0
        if C == 2:                # (for C > 2 the foreground's 1 - 1 / C comes before the background's 1 / C, each in pixel order)
            for grp in LV.segments(B, per_image):
                for c in range(C):
                    assert np.array_equal(np.concatenate([ranks[c, b].reshape(-1).numpy() for b in grp]), np.arange(len(grp) * H * W))
        assert abs(float(v) - (1.0 - 1.0 / C)) <= LV.CAP["value"]
    if kind == "low_digit":       # all errors share the key's upper twenty bits
        assert len(np.unique(bits >> 10)) == 1 and len(np.unique(bits & 0x3FF)) > 100
    if kind == "high_digit":      # ... or its lower twenty
        assert (bits & 0xFFFFF == 0).all() and len(np.unique(bits >> 20)) >= 4 and ties > 0
    if kind in ("c1", "all_ignored"):
        assert float(v) == 0.0 and float(grad.abs().max()) == 0.0
    if kind == "all_ignored":
        assert bool((ranks == -1).all())


@pytest.mark.parametrize("tag", LV.LAYOUT_TAGS)
def test_layouts(cuda, tag):
    """NCHW, NHWC, the first channels of an 8-channel NHWC tensor, a crop: the same ranks, the same gradient within the bar"""
    base = None
    for name in LV.LAYOUTS:
        v, grad, errors, ranks = run_case(cuda, tag, name)
        if base is None:
            base = (v, grad.clone(), ranks)
            ref = LV.reference(tag, T, ranks.numpy())
        what = f"lovasz {tag} {name}"
        assert torch.equal(ranks, base[2]), what
        ref.check("value", v, LV.CAP["value"], what)
        ref.check("grad", grad, LV.CAP["grad"], what)
        assert LV.err_of("grad", grad, base[1]) <= ref.bar("grad", LV.CAP["grad"]), what
    mgunet.losses.check_labels(cuda)


@pytest.mark.parametrize("tag", LV.RAW_TAGS)
def test_backward_accumulate_raw_abi(cuda, tag):
    """mgu_lovasz_softmax_backward as Trainer(loss="ce+lovasz") calls it: adding into a prefilled destination of pitch 8, grad_scale
    together with grad_scale_dev, the loss written by the same call; channels [C, 8) keep their bytes"""
    B, C, H, W, _, classes, per_image = LV.cases(T)[tag]
    HW, pitch = H * W, LV.RAW_PITCH
    lg, y, _, _ = LV.inputs(tag, T)
    lgd, yd = lg.to(cuda).contiguous(), y.to(cuda).contiguous()
    _, _, ranks = _lovasz_debug(lgd, yd, classes=classes, per_image=per_image)
    pre = LV.raw_prefill(tag, T).to(cuda)
    dst = pre.clone()
    scale_dev = torch.tensor([LV.RAW_SCALE_DEV], device=cuda, dtype=torch.float32)
    loss = torch.full((), -5.0, device=cuda, dtype=torch.float32)
    _lib.call("mgu_lovasz_softmax_backward", cuda, lgd, yd, B, HW, C, C * HW, HW, 1, int(classes == "all"), int(per_image), LV.IGNORE,
              LV.RAW_SCALE, scale_dev, dst, HW * pitch, 1, pitch, 1, loss)
    ref = LV.raw_reference(tag, T, ranks.cpu().numpy())
    ref.check("acc", dst[:, :C], LV.CAP["grad"], f"lovasz accumulate {tag}")
    ref.check("value", loss, LV.CAP["value"], f"lovasz accumulate {tag}")
    assert torch.equal(dst[:, C:], pre[:, C:])
    mgunet.losses.check_labels(cuda)


def test_bad_label_gives_nan_and_is_reported(cuda):
    lg, y, _, _ = LV.inputs("ignore", T)
    assert bool((y == LV.IGNORE).any())
    v = mgunet.lovasz_softmax(lg.to(cuda), y.to(cuda))
    assert bool(torch.isfinite(v))
    mgunet.losses.check_labels(cuda)                                # -100 is no bad label
    y = y.clone()
    y[1, 3, 4] = 9
    v = mgunet.lovasz_softmax(lg.to(cuda), y.to(cuda))
    assert bool(torch.isnan(v))
    with pytest.raises(ValueError, match="label outside"):
        mgunet.losses.check_labels(cuda)
    mgunet.losses.check_labels(cuda)                                # reported once


def test_nine_classes_and_empty_shapes_raise_and_launch_nothing(cuda):
    y = torch.zeros(1, 4, 4, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="num_classes <= 8"):
        mgunet.lovasz_softmax(torch.zeros(1, 9, 4, 4, device=cuda, requires_grad=True), y)
    with pytest.raises(ValueError, match="present"):
        mgunet.lovasz_softmax(torch.zeros(1, 2, 4, 4, device=cuda), y, classes="some")
    lg = torch.zeros(1, 9, 4, 4, device=cuda)
    loss = torch.full((), -5.0, device=cuda)
    errors, ranks = torch.full((9, 16), -5.0, device=cuda), torch.full((9, 16), -5, device=cuda, dtype=torch.int32)
    dst = torch.full((16, 12), -5.0, device=cuda)
    one = torch.ones(1, device=cuda)
    for C, HW in ((9, 16), (2, 0)):
        with pytest.raises(ValueError, match="num_classes <= 8"):
            _lib.call("mgu_lovasz_softmax", cuda, lg, y, 1, HW, C, C * 16, 16, 1, 0, 0, LV.IGNORE, loss, errors, ranks)
        with pytest.raises(ValueError, match="num_classes <= 8"):
            _lib.call("mgu_lovasz_softmax_backward", cuda, lg, y, 1, HW, C, C * 16, 16, 1, 0, 0, LV.IGNORE, 1.0, one, dst, 16 * 12, 1, 12, 0, loss)
    torch.cuda.synchronize(cuda)
    assert float(loss) == -5.0 and bool((errors == -5.0).all()) and bool((ranks == -5).all()) and bool((dst == -5.0).all())


def test_two_calls_are_bitwise_equal(cuda):
    tag = f"n{3 * T + 5}"
    a, b = run_case(cuda, tag), run_case(cuda, tag)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3]) and torch.equal(a[2], b[2])


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
CFG = (3, 3, 8, 2)
# (kernel family, launches) of one Trainer(loss="ce").forward_backward at 2 x 32 x 32 with profiling on, in order of first launch, as
# recorded on the code path before the Lovasz loss was added
CE_LAUNCHES = [("igemm_kernel<f32>", 4), ("wino3x3_cp_kernel<1>", 6), ("igemm_kernel<f32> (ConvTranspose)", 2), ("wgrad (direct) kernels", 9),
               ("igemm/halo (dgrad)", 4), ("igemm_kernel<f32> (ConvTranspose dgrad)", 2), ("wino3x3_cp_kernel<1> (dgrad)", 5),
               ("wino_wgrad_f32_kernel<X3>", 1)]


def build_trainer(cuda, **kw):
    model = mgunet.UNet(*CFG)
    model.load_state_dict(O.make_unet_params(*CFG, seed=61))
    return mgunet.Trainer(model.to(cuda), comm=None, **kw)


def trainer_batch(cuda):
    x = torch.from_numpy(O.formula_normal("lovasz/tr/x", (2, 3, 32, 32), seed=62)).to(cuda)
    y = torch.from_numpy(O.formula_labels("lovasz/tr/y", (2, 32, 32), CFG[1], seed=63)).clone()
    y[0, :4] = LV.IGNORE
    return x, y.to(cuda)


@pytest.mark.parametrize("kw", [{}, {"lovasz_per_image": True, "lovasz_classes": "all"}, {"loss": "ce+dice+lovasz"}],
                         ids=["batch", "per_image_all", "with_dice"])
def test_trainer_ce_plus_lovasz_is_the_composition(cuda, kw):
    x, y = trainer_batch(cuda)
    kw = dict(kw)
    kind = kw.pop("loss", "ce+lovasz")
    if "dice" in kind:                                              # dice flags -100 as a bad label: no ignored pixels here
        y = y.clamp_min(0)
    tr = build_trainer(cuda, loss=kind, **kw)
    loss = tr.forward_backward(x, y).clone()
    # by hand on a second, identical trainer's context
    t2 = build_trainer(cuda, loss="ce")
    ctx = t2.model._context(cuda)
    t2.model.train()
    logits, _, _ = t2.model(x)
    B, Cc, H, W = logits.shape
    nhwc = logits.permute(0, 2, 3, 1)
    assert nhwc.is_contiguous()
    npix, ldd = B * H * W, (Cc + 3) // 4 * 4
    dlogits = torch.empty((npix, ldd), device=cuda)
    ce, dc, lv = torch.zeros(1, device=cuda), torch.zeros(1, device=cuda), torch.zeros(1, device=cuda)
    _lib.call("mgu_cross_entropy", cuda, nhwc, y, npix, Cc, 1.0 / npix, dlogits, ce, ctx=ctx)
    if "dice" in kind:
        _lib.call("mgu_dice_loss_backward", cuda, nhwc, y, B, H * W, Cc, H * W * Cc, 1, Cc, 1.0, 1.0, None, dlogits, H * W * ldd, 1, ldd, 1, dc,
                  ctx=ctx)
    _lib.call("mgu_lovasz_softmax_backward", cuda, nhwc, y, B, H * W, Cc, H * W * Cc, 1, Cc, int(kw.get("lovasz_classes") == "all"),
              int(kw.get("lovasz_per_image", False)), LV.IGNORE, 1.0, None, dlogits, H * W * ldd, 1, ldd, 1, lv, ctx=ctx)
    _lib.call("mgu_unet_backward", cuda, dlogits, t2.grad, ctx=ctx)
    assert torch.equal(loss, (ce + dc + lv) if "dice" in kind else (ce + lv)) and float(lv) > 0.0
    assert torch.equal(tr.grad, t2.grad)
    # the loss it adds is the public function's on the same logits
    pub = mgunet.lovasz_softmax(logits.detach(), y, classes=kw.get("lovasz_classes", "present"), per_image=kw.get("lovasz_per_image", False))
    assert torch.equal(pub.reshape(1), lv)
    tr.check()


def test_trainer_ce_takes_the_calls_it_took(cuda):
    """Trainer(loss="ce") beside a "ce+lovasz" trainer: the launches of its step are the recorded list, its gradient the composition
    of mgu_cross_entropy and mgu_unet_backward alone, bitwise"""
    x, y = trainer_batch(cuda)
    build_trainer(cuda, loss="ce+lovasz").forward_backward(x, y)
    tr = build_trainer(cuda, loss="ce")
    ctx, L = tr.model._context(cuda), _lib.lib()
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        loss = tr.forward_backward(x, y).clone()
        torch.cuda.synchronize(cuda)
        names = [(k["name"], k["launches"]) for k in _lib.read_kernel_stats(ctx)]
    finally:
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    assert names == CE_LAUNCHES
    t2 = build_trainer(cuda, loss="ce")
    t2.model.train()
    logits, _, _ = t2.model(x)
    B, Cc, H, W = logits.shape
    npix, ldd = B * H * W, (Cc + 3) // 4 * 4
    dlogits = torch.empty((npix, ldd), device=cuda)
    ce = torch.zeros(1, device=cuda)
    c2 = t2.model._context(cuda)
    _lib.call("mgu_cross_entropy", cuda, logits.permute(0, 2, 3, 1), y, npix, Cc, 1.0 / npix, dlogits, ce, ctx=c2)
    _lib.call("mgu_unet_backward", cuda, dlogits, t2.grad, ctx=c2)
    assert torch.equal(loss, ce) and torch.equal(tr.grad, t2.grad)
