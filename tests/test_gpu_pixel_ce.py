"""The pixel cross-entropy kernels (csrc/pixel_ce.hip) on the GPU: the radix select against the tie rule (exact, on the device's own
fp32 losses), value and gradient against float64 with the device's own kept map pinned, at the group sizes around the workgroup
tile, at the key's edges (one giant tie, a tie across a tile boundary, losses of exactly +0, losses that differ in the lowest / the
highest digit only, K = 1), every class count, every option alone and combined, every storage layout, the raw ABI as the trainer
calls it, bad labels and limits, bitwise reproducibility, the launch counts, and Trainer with the new options.

Cases, reference and bars: tests/pixel_ce_cases.py (bar = 4 * cond + 2^-22, cond = the same code in fp32 under the same pinned kept
map; caps 2e-6 for the value, 5e-6 for gradients and for the per-pixel loss plane).  NOTES.md ("Pixel cross-entropy: float64 bars")
carries the lines these tests print under -s."""
import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
import pixel_ce_cases as PC
from mgunet import _lib
from mgunet.losses import _pixel_ce_debug

pytestmark = pytest.mark.gpu

T = 4096            # mgu_pixel_ce_tile() of the library this suite was written against; test_tile_size holds the two together
ALL_TAGS = list(PC.cases(T))
LAUNCHES = {False: (2, 3), True: (8, 9)}      # the header's statement: select off / on -> (value, value + gradient)


def leaf(view):
    return view.detach().requires_grad_(True)


def run_case(cuda, tag, layout="nchw", **override):
    """(value, gradient, pixel_loss, kept) of the device for the case, the last two on the host"""
    lg, y, opt = PC.inputs(tag, T)
    opt = dict(opt, **override)
    yd = y.to(cuda)
    l = leaf(PC.LAYOUTS[layout](lg.to(cuda)))
    kw = PC.api_kwargs(opt, cuda)
    v = mgunet.pixel_cross_entropy(l, yd, **kw)
    v.backward()
    dv, plane, kept = _pixel_ce_debug(l.detach(), yd, **kw)
    assert torch.equal(dv, v.detach())                              # the hooks change nothing
    return v.detach(), l.grad, plane.cpu(), kept.cpu()


def test_tile_size(cuda):
    assert int(_lib.lib().mgu_pixel_ce_tile()) == T


@pytest.mark.parametrize("tag", ALL_TAGS)
def test_selection_value_and_gradient(cuda, tag):
    B, C, H, W, kind, opt = PC.cases(T)[tag]
    lg, y, _ = PC.inputs(tag, T)
    v, grad, plane, kept = run_case(cuda, tag)
    mgunet.losses.check_labels(cuda)
    what = f"pixel_ce {tag} ({B}x{C}x{H}x{W})"
    counted = (y != PC.IGNORE).numpy()
    # 1. the select: exact against the oracle run on the device's own losses; the losses against float64
    assert tuple(plane.shape) == tuple(kept.shape) == (B, H, W) and kept.dtype == torch.int32
    want = PC.select(plane.numpy(), counted, opt["keep"], opt["min_kept"], opt["per_image"])
    assert np.array_equal(kept.numpy(), want), what
    assert float(plane.min()) >= 0.0 and not bool(np.signbit(plane.numpy()).any()) and float(plane[torch.as_tensor(~counted)].abs().sum()) == 0.0
    PC.plane_reference(tag, T).check("plane", plane, PC.CAP["plane"], what)
    for grp in PC.groups(B, opt["per_image"]):
        n = int(sum(counted[b].sum() for b in grp))
        K = n if opt["keep"] == 1.0 else PC.kept_count(n, opt["keep"], opt["min_kept"])
        assert int(sum((kept[b] == 1).sum() for b in grp)) == K, (what, grp)
    # 2. value and every element of the gradient with that kept map pinned
    ref = PC.reference(tag, T, kept.numpy())
    ref.check("value", v, PC.CAP["value"], what)
    ref.check("grad", grad, PC.CAP["grad"], what)
    if opt["weight"] is None:                                       # the value is continuous across a swap: the reference's own selection
        free = PC.reference(tag, T)
        assert PC.err_of("value", v, free.r64["value"]) <= ref.bar("value", PC.CAP["value"]), what
    assert tuple(grad.shape) == (B, C, H, W) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(v))
    off = torch.as_tensor(kept.numpy() != 1).to(cuda)               # ignored and dropped pixels get exactly no gradient
    if bool(off.any()):
        assert float(grad.permute(0, 2, 3, 1)[off].abs().max()) == 0.0
    # 3. what the case is there for
    bits = plane.numpy().view(np.uint32).reshape(-1)
    flat = kept.numpy().reshape(-1)
    if kind == "equal":           # one tie over every group: kept = its first K pixels exactly, and K falls inside the tie
        assert len(np.unique(bits)) == 1
        for grp in PC.groups(B, opt["per_image"]):
            k = np.concatenate([kept[b].reshape(-1).numpy() for b in grp])
            K = int((k == 1).sum())
            assert 0 < K < len(k) and (k[:K] == 1).all() and (k[K:] == 0).all()
    if kind == "straddle":        # the tie's first 180 pixels are kept: 100 before the tile boundary, 80 behind it
        r = opt["min_kept"] - PC.STRADDLE_HARD
        lo = T - PC.STRADDLE_TIE[0]
        assert len(np.unique(bits[lo:T + PC.STRADDLE_TIE[1]])) == 1
        assert (flat[lo:lo + r] == 1).all() and (flat[lo + r:T + PC.STRADDLE_TIE[1]] == 0).all() and lo + r > T
        assert int((flat == 1).sum()) == opt["min_kept"]
    if kind == "saturated":       # losses exactly +0 beside 120
        assert set(np.unique(bits)) == {0, np.float32(120.0).view(np.uint32)}
        zero_kept = int(((flat == 1) & (bits == 0)).sum())
        assert (zero_kept > 0) == (tag == "saturated_zero")
    if kind == "low_digit":       # all losses share the key's upper 24 bits, up to one carry
        assert len(np.unique(bits >> 7)) <= 2 and len(np.unique(bits & 0x7F)) > 50
    if kind == "high_digit":      # ... or differ in its top digit only
        assert (bits & 0x7FFFFF == 0).all() and len(np.unique(bits >> 23)) == 5
    if tag == "k1":
        assert int((flat == 1).sum()) == 1 and int(np.argmax(flat == 1)) == int(np.argmax(plane.numpy().reshape(-1)))
    if C == 1:
        assert float(v) == 0.0 and float(grad.abs().max()) == 0.0
    if kind == "sure":            # p_y exactly 1: loss +0 and a zero row, under gamma = 1 too
        sure = (bits == 0) & counted.reshape(-1)
        assert int(sure.sum()) > 20
        assert float(grad.permute(0, 2, 3, 1).reshape(-1, C)[torch.as_tensor(sure).to(cuda)].abs().max()) == 0.0


def test_min_kept_above_the_count_keeps_all_bitwise_as_without_mining(cuda):
    for tag in ("opt_weights_smooth", "opt_focal2", "n4097", "image_of_3"):
        n = int(np.prod(PC.cases(T)[tag][:1] + PC.cases(T)[tag][2:4]))
        full = run_case(cuda, tag, keep=1.0, min_kept=0)
        mined = run_case(cuda, tag, keep=0.25, min_kept=n)
        assert bool((full[3] != 0).all()) and torch.equal(full[3], mined[3])
        assert torch.equal(full[0], mined[0]) and torch.equal(full[1], mined[1]) and torch.equal(full[2], mined[2]), tag


@pytest.mark.parametrize("tag", PC.LAYOUT_TAGS)
def test_layouts(cuda, tag):
    """NCHW, NHWC, the first channels of an 8-channel NHWC tensor, a crop: the same kept map, the same gradient within the bar"""
    base = None
    for name in PC.LAYOUTS:
        v, grad, plane, kept = run_case(cuda, tag, name)
        if base is None:
            base = (v, grad.clone(), kept)
            ref = PC.reference(tag, T, kept.numpy())
        what = f"pixel_ce {tag} {name}"
        assert torch.equal(kept, base[2]), what
        ref.check("value", v, PC.CAP["value"], what)
        ref.check("grad", grad, PC.CAP["grad"], what)
        assert PC.err_of("grad", grad, base[1]) <= ref.bar("grad", PC.CAP["grad"]), what
    mgunet.losses.check_labels(cuda)


def raw_args(cuda, tag):
    B, C, H, W, _, opt = PC.cases(T)[tag]
    lg, y, _ = PC.inputs(tag, T)
    kw = PC.api_kwargs(opt, cuda)
    return (B, C, H * W, opt, lg.to(cuda).contiguous(), y.to(cuda).contiguous(), kw,
            (kw["weight"], opt["eps"], opt["gamma"], opt["keep"], opt["min_kept"], int(opt["per_image"]), PC.IGNORE))


@pytest.mark.parametrize("tag", PC.RAW_TAGS)
def test_backward_raw_abi_as_the_trainer_calls_it(cuda, tag):
    """mgu_pixel_ce_backward on a destination of pitch 8: accumulate = 0 with zero_to = 8 writes every column (the padding ones 0),
    accumulate = 1 adds into a prefilled buffer and leaves the padding columns alone; grad_scale together with grad_scale_dev, the
    loss written by the same call"""
    B, C, HW, opt, lgd, yd, kw, tail = raw_args(cuda, tag)
    pitch = PC.RAW_PITCH
    _, _, kept = _pixel_ce_debug(lgd, yd, **kw)
    kept = kept.cpu().numpy()
    scale_dev = torch.tensor([PC.RAW_SCALE_DEV], device=cuda, dtype=torch.float32)
    for accumulate in (1, 0):
        pre = PC.raw_prefill(tag, T).to(cuda)
        dst = pre.clone()
        loss = torch.full((), -5.0, device=cuda, dtype=torch.float32)
        _lib.call("mgu_pixel_ce_backward", cuda, lgd, yd, B, HW, C, C * HW, HW, 1, *tail, PC.RAW_SCALE, scale_dev, dst, HW * pitch, 1, pitch,
                  accumulate, pitch, loss)
        ref = PC.raw_reference(tag, T, kept, bool(accumulate))
        what = f"pixel_ce raw {tag} accumulate={accumulate}"
        ref.check("acc", dst[:, :C], PC.CAP["grad"], what)
        ref.check("value", loss, PC.CAP["value"], what)
        if accumulate:
            assert torch.equal(dst[:, C:], pre[:, C:])
            off = torch.as_tensor(kept.reshape(-1) != 1).to(cuda)           # nothing is added to a pixel that is not kept
            assert torch.equal(dst[off], pre[off])
        else:
            assert float(dst[:, C:].abs().max()) == 0.0
    # zero_to = 0 without accumulate: the padding columns keep their bytes
    pre = PC.raw_prefill(tag, T).to(cuda)
    dst = pre.clone()
    _lib.call("mgu_pixel_ce_backward", cuda, lgd, yd, B, HW, C, C * HW, HW, 1, *tail, 1.0, None, dst, HW * pitch, 1, pitch, 0, 0, None)
    assert torch.equal(dst[:, C:], pre[:, C:])
    mgunet.losses.check_labels(cuda)


@pytest.mark.parametrize("mined", [False, True])
def test_bad_label_gives_nan_and_is_reported(cuda, mined):
    lg, y, opt = PC.inputs("opt_plain_mined" if mined else "opt_plain", T)
    kw = PC.api_kwargs(opt, cuda)
    assert bool((y == PC.IGNORE).any())
    v = mgunet.pixel_cross_entropy(lg.to(cuda), y.to(cuda), **kw)
    assert bool(torch.isfinite(v))
    mgunet.losses.check_labels(cuda)                                # -100 is no bad label
    y = y.clone()
    y[1, 3, 4] = 9
    l = leaf(lg.to(cuda))
    v = mgunet.pixel_cross_entropy(l, y.to(cuda), **kw)
    v.backward()
    assert bool(torch.isnan(v))
    assert float(l.grad[1, :, 3, 4].abs().max()) == 0.0             # and is never used as an index
    with pytest.raises(ValueError, match="label outside"):
        mgunet.losses.check_labels(cuda)
    mgunet.losses.check_labels(cuda)                                # reported once
    _, _, kept = _pixel_ce_debug(lg.to(cuda), y.to(cuda), **kw)
    assert int(kept[1, 3, 4]) == -1
    with pytest.raises(ValueError, match="label outside"):
        mgunet.losses.check_labels(cuda)
    # another ignore_index: the label 9 is skipped, -100 is now the bad one and there is none left
    y2 = torch.where(y == PC.IGNORE, torch.full_like(y, 9), y)
    v2 = mgunet.pixel_cross_entropy(lg.to(cuda), y2.to(cuda), ignore_index=9, **kw)
    assert bool(torch.isfinite(v2))
    mgunet.losses.check_labels(cuda)


def test_no_counted_pixel_gives_nan_and_zero_gradient(cuda):
    for keep in (1.0, 0.25):
        l = leaf(torch.zeros(2, 3, 5, 7, device=cuda))
        v = mgunet.pixel_cross_entropy(l, torch.full((2, 5, 7), PC.IGNORE, device=cuda), keep_fraction=keep)
        v.backward()
        assert bool(torch.isnan(v)) and float(l.grad.abs().max()) == 0.0
    mgunet.losses.check_labels(cuda)


def test_limits_raise_and_launch_nothing(cuda):
    y = torch.zeros(1, 4, 4, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="num_classes <= 8"):
        mgunet.pixel_cross_entropy(torch.zeros(1, 9, 4, 4, device=cuda, requires_grad=True), y)
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.pixel_cross_entropy(torch.zeros(1, 2, 4, 4), y.cpu())
    lg = torch.zeros(1, 9, 4, 4, device=cuda)
    loss = torch.full((), -5.0, device=cuda)
    plane, kept = torch.full((16,), -5.0, device=cuda), torch.full((16,), -5, device=cuda, dtype=torch.int32)
    dst = torch.full((16, 12), -5.0, device=cuda)
    one = torch.ones(1, device=cuda)
    ok = dict(C=2, HW=16, eps=0.0, gamma=0.0, keep=0.5, min_kept=0)
    bad = [({"C": 9}, "num_classes <= 8"), ({"HW": 0}, "num_classes <= 8"), ({"eps": 1.0}, "label_smoothing"), ({"eps": -0.5}, "label_smoothing"),
           ({"gamma": 0.5}, "focal_gamma"), ({"gamma": -2.0}, "focal_gamma"), ({"gamma": 2.0, "eps": 0.1}, "label_smoothing"),
           ({"keep": 0.0}, "keep_fraction"), ({"keep": 1.5}, "keep_fraction"), ({"min_kept": -1}, "min_kept")]
    ctx = _lib.context(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        for change, match in bad:
            a = dict(ok, **change)
            mid = (None, a["eps"], a["gamma"], a["keep"], a["min_kept"], 0, PC.IGNORE)
            with pytest.raises(ValueError, match=match):
                _lib.call("mgu_pixel_ce", cuda, lg, y, 1, a["HW"], a["C"], a["C"] * 16, 16, 1, *mid, loss, plane, kept)
            with pytest.raises(ValueError, match=match):
                _lib.call("mgu_pixel_ce_backward", cuda, lg, y, 1, a["HW"], a["C"], a["C"] * 16, 16, 1, *mid, 1.0, one, dst, 16 * 12, 1, 12, 0, 12, loss)
        with pytest.raises(ValueError, match="2\\^30"):
            _lib.call("mgu_pixel_ce", cuda, lg, y, 1 << 15, 1 << 15, 2, 2 << 15, 1 << 15, 1, None, 0.0, 0.0, 0.5, 0, 0, PC.IGNORE, loss, plane, kept)
        torch.cuda.synchronize(cuda)
        assert _lib.read_kernel_stats(ctx) == []
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    assert float(loss) == -5.0 and bool((plane == -5.0).all()) and bool((kept == -5).all()) and bool((dst == -5.0).all())


def test_two_calls_are_bitwise_equal(cuda):
    for tag in (f"n{2 * T + 17}", "image_of_3_weights", "equal"):
        a, b = run_case(cuda, tag), run_case(cuda, tag)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), tag


def count_launches(cuda, B, C, keep, backward, per_image=False):
    lg = torch.from_numpy(O.formula_normal("pce/launch/l", (B, C, 9, 11), seed=C)).to(cuda)
    y = torch.from_numpy(O.formula_labels("pce/launch/y", (B, 9, 11), C, seed=B)).to(cuda)
    ctx = _lib.context(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        if backward:
            mgunet.pixel_cross_entropy(leaf(lg), y, keep_fraction=keep, per_image=per_image)          # the value's launches ...
            torch.cuda.synchronize(cuda)
            _lib.read_kernel_stats(ctx)
            l = leaf(lg)
            v = mgunet.pixel_cross_entropy(l, y, keep_fraction=keep, per_image=per_image)
            torch.cuda.synchronize(cuda)
            _lib.read_kernel_stats(ctx)
            v.backward()                                                                              # ... and the backward entry's alone
        else:
            mgunet.pixel_cross_entropy(lg, y, keep_fraction=keep, per_image=per_image)
        torch.cuda.synchronize(cuda)
        stats = _lib.read_kernel_stats(ctx)
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    assert all(k["name"].startswith("pixel_ce") for k in stats), stats
    return sum(k["launches"] for k in stats)


@pytest.mark.parametrize("select", [False, True])
def test_launch_counts_are_fixed_and_as_stated(cuda, select):
    keep = 0.25 if select else 1.0
    for backward in (False, True):
        got = {(B, C, pi): count_launches(cuda, B, C, keep, backward, pi) for B in (1, 3) for C in (2, 8) for pi in (False, True)}
        assert set(got.values()) == {LAUNCHES[select][int(backward)]}, (select, backward, got)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
CFG = (3, 3, 8, 2)


def build_trainer(cuda, **kw):
    model = mgunet.UNet(*CFG)
    model.load_state_dict(O.make_unet_params(*CFG, seed=61))
    return mgunet.Trainer(model.to(cuda), comm=None, **kw)


def trainer_batch(cuda):
    x = torch.from_numpy(O.formula_normal("pce/tr/x", (2, 3, 32, 32), seed=62)).to(cuda)
    y = torch.from_numpy(O.formula_labels("pce/tr/y", (2, 32, 32), CFG[1], seed=63)).clone()
    y[0, :4] = PC.IGNORE
    return x, y.to(cuda)


TRAINER_KW = {
    "weights": {"ce_weight": (0.5, 2.0, 1.25)},
    "smooth_mined_image": {"label_smoothing": 0.1, "hard_fraction": 0.25, "hard_min_kept": 100, "hard_per_image": True},
    "focal_mined": {"focal_gamma": 2.0, "hard_fraction": 0.3},
    "all_with_dice": {"ce_weight": (0.5, 2.0, 0.0), "label_smoothing": 0.1, "hard_fraction": 0.5, "loss": "ce+dice"},
    "mined_with_lovasz": {"hard_fraction": 0.25, "loss": "ce+lovasz"},
}


@pytest.mark.parametrize("name", list(TRAINER_KW))
def test_trainer_with_the_new_options_is_the_composition(cuda, name):
    x, y = trainer_batch(cuda)
    kw = dict(TRAINER_KW[name])
    kind = kw.pop("loss", "ce")
    if "dice" in kind:                                              # dice flags -100 as a bad label: no ignored pixels here
        y = y.clamp_min(0)
    if "ce_weight" in kw:
        kw["ce_weight"] = torch.tensor(kw["ce_weight"])
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
    dlogits = torch.full((npix, ldd), 7.0, device=cuda)
    ce, dc, lv = torch.zeros(1, device=cuda), torch.zeros(1, device=cuda), torch.zeros(1, device=cuda)
    w = kw["ce_weight"].to(cuda) if "ce_weight" in kw else None
    mid = (w, kw.get("label_smoothing", 0.0), kw.get("focal_gamma", 0.0), kw.get("hard_fraction", 1.0), kw.get("hard_min_kept", 0),
           int(kw.get("hard_per_image", False)), PC.IGNORE)
    _lib.call("mgu_pixel_ce_backward", cuda, nhwc, y, B, H * W, Cc, H * W * Cc, 1, Cc, *mid, 1.0, None, dlogits, H * W * ldd, 1, ldd, 0, ldd, ce,
              ctx=ctx)
    assert float(dlogits[:, Cc:].abs().max()) == 0.0 and float(dlogits[:, :Cc].abs().max()) > 0.0
    if "dice" in kind:
        _lib.call("mgu_dice_loss_backward", cuda, nhwc, y, B, H * W, Cc, H * W * Cc, 1, Cc, 1.0, 1.0, None, dlogits, H * W * ldd, 1, ldd, 1, dc,
                  ctx=ctx)
    if "lovasz" in kind:
        _lib.call("mgu_lovasz_softmax_backward", cuda, nhwc, y, B, H * W, Cc, H * W * Cc, 1, Cc, 0, 0, PC.IGNORE, 1.0, None, dlogits,
                  H * W * ldd, 1, ldd, 1, lv, ctx=ctx)
    _lib.call("mgu_unet_backward", cuda, dlogits, t2.grad, ctx=ctx)
    want = ce + dc if "dice" in kind else (ce + lv if "lovasz" in kind else ce)
    assert torch.equal(loss, want) and float(ce) > 0.0
    assert torch.equal(tr.grad, t2.grad) and float(tr.grad.abs().max()) > 0.0
    # the term is the public function's on the same logits
    pub = mgunet.pixel_cross_entropy(logits.detach(), y, weight=w, label_smoothing=mid[1], focal_gamma=mid[2], keep_fraction=mid[3],
                                     min_kept=mid[4], per_image=bool(mid[5]))
    assert torch.equal(pub.reshape(1), ce)
    tr.check()


def test_trainer_with_default_options_beside_it_is_the_plain_composition(cuda):
    x, y = trainer_batch(cuda)
    build_trainer(cuda, hard_fraction=0.25, ce_weight=torch.tensor([0.5, 2.0, 1.25])).forward_backward(x, y)
    tr = build_trainer(cuda, ce_weight=None, label_smoothing=0.0, focal_gamma=0.0, hard_fraction=1.0, hard_min_kept=0, hard_per_image=False)
    assert tr.pixel_ce is None
    ctx, L = tr.model._context(cuda), _lib.lib()
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        loss = tr.forward_backward(x, y).clone()
        torch.cuda.synchronize(cuda)
        names = [k["name"] for k in _lib.read_kernel_stats(ctx)]
    finally:
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    assert names and not any(n.startswith("pixel_ce") for n in names)
    t2 = build_trainer(cuda)
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
    # with a mining trainer the profile of the same step does name the new kernels
    t3 = build_trainer(cuda, hard_fraction=0.25)
    c3 = t3.model._context(cuda)
    _lib.check(L.mgu_profile_enable(c3.handle, 1), c3.handle)
    try:
        t3.forward_backward(x, y)
        torch.cuda.synchronize(cuda)
        stats = _lib.read_kernel_stats(c3)
    finally:
        _lib.check(L.mgu_profile_enable(c3.handle, 0), c3.handle)
    assert sum(k["launches"] for k in stats if k["name"].startswith("pixel_ce")) == LAUNCHES[True][1]
