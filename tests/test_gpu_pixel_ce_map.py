"""The pixel cross-entropy with a per-pixel weight map (mgu_pixel_ce_map / mgu_pixel_ce_map_backward, csrc/pixel_ce.hip) on the GPU, and
Trainer's border weight map.  The inputs, the float64 reference and the bars are tests/pixel_ce_cases.py's, unchanged: the reference
is extended here by the map m (loss m l per pixel, L = sum_kept m l / sum_kept m w_y, m held fixed), the bar stays 4 * cond + 2^-22
with cond the same expression in fp32 under the device's own pinned kept map, the caps 2e-6 for the value and 5e-6 for the
gradient and the loss plane.  A NULL map and a map of ones must give the bits of the entries without a map.
NOTES.md ("Border weight map") carries the lines these tests print under -s."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
import pixel_ce_cases as PC
from mgunet import _lib
from mgunet.losses import _pixel_ce_debug

pytestmark = pytest.mark.gpu

T = 4096            # mgu_pixel_ce_tile(): tests/test_gpu_pixel_ce.py::test_tile_size holds the library to it
TAGS = (f"n{T - 1}", f"n{T}", f"n{T + 1}", "equal", "equal_image", "straddle", "image_of_3_weights", "opt_weights_smooth_mined", "opt_focal2",
        "opt_all_image", "c6")
MAPS = ("ones", "random", "border", "zeros")
LAUNCHES = {False: (2, 3), True: (8, 9)}


@lru_cache(maxsize=None)
def host_map(tag, kind):
    """the map of a case on the host, float32 (B, H, W); "border" is made on the device (device_map)"""
    B, C, H, W = PC.cases(T)[tag][:4]
    if kind == "ones":
        return torch.ones(B, H, W)
    u = torch.from_numpy(O.formula_uniform(f"pcemap/{tag}/{kind}", (B, H, W), seed=17)).float()
    if kind == "random":
        return (0.5 + 10.5 * u).contiguous()
    z = torch.from_numpy(O.formula_uniform(f"pcemap/{tag}/z", (B, H, W), seed=18))
    return torch.where(z < 0.3, torch.zeros(()), 0.5 + 2.0 * u).contiguous()       # "zeros": three pixels in ten carry no weight


def device_map(cuda, tag, kind):
    if kind != "border":
        return host_map(tag, kind).to(cuda)
    _, y, _ = PC.inputs(tag, T)
    lab = y.clamp_min(0).to(torch.int32).to(cuda)              # the classes as instances: a real border_weights map of the case's shape
    return mgunet.border_weights(lab, classes=y.to(cuda), class_weight=torch.tensor([1.0, 0.5, 2.0, 1.5, 1.0, 1.0, 1.0, 1.0]), w0=10.0, sigma=3.0)


def map_reference(tag, m, kept) -> PC.Ref:
    """value and dlogits in float64 (and cond from fp32) with the map and the given kept map pinned"""
    lg, y, opt = PC.inputs(tag, T)

    def loss(l, dt):
        pl, wy, _ = PC.pixel_losses(l, y, opt, PC.IGNORE, dt)
        k = torch.as_tensor(np.asarray(kept) == 1)
        md, zero = m.to(dt), torch.zeros((), dtype=dt)
        return torch.where(k, md * pl, zero).sum() / torch.where(k, md * wy, zero).sum()
    return PC.Ref(lambda dt: PC.autograd_run(lambda l: loss(l, dt), [lg], dt, names=["grad"]))


def run(cuda, tag, m, layout="nchw"):
    """(value, gradient, plane, kept) of the device with the map m (a device tensor or None)"""
    lg, y, opt = PC.inputs(tag, T)
    yd = y.to(cuda)
    l = PC.LAYOUTS[layout](lg.to(cuda)).detach().requires_grad_(True)
    kw = PC.api_kwargs(opt, cuda)
    v = mgunet.pixel_cross_entropy(l, yd, pixel_weight=m, **kw)
    v.backward()
    dv, plane, kept = _pixel_ce_debug(l.detach(), yd, pixel_weight=m, **kw)
    assert torch.equal(dv, v.detach())
    return v.detach(), l.grad, plane.cpu(), kept.cpu()


@pytest.mark.parametrize("tag", TAGS)
def test_null_map_and_ones_are_the_entries_without_a_map(cuda, tag):
    base = run(cuda, tag, None)
    ones = run(cuda, tag, device_map(cuda, tag, "ones"))
    assert all(torch.equal(a, b) for a, b in zip(base, ones)), tag
    # the raw entries with a NULL map
    B, C, H, W, _, opt = PC.cases(T)[tag]
    lg, y, _ = PC.inputs(tag, T)
    lgd, yd, kw = lg.to(cuda).contiguous(), y.to(cuda), PC.api_kwargs(opt, cuda)
    tail = (opt["eps"], opt["gamma"], opt["keep"], opt["min_kept"], int(opt["per_image"]), PC.IGNORE)
    got = []
    for name, extra in (("mgu_pixel_ce", ()), ("mgu_pixel_ce_map", (None,))):
        loss = torch.zeros((), device=cuda)
        plane, kept = torch.empty((B, H, W), device=cuda), torch.empty((B, H, W), device=cuda, dtype=torch.int32)
        d = torch.empty((B, C, H, W), device=cuda)
        loss2 = torch.zeros((), device=cuda)
        _lib.call(name, cuda, lgd, yd, B, H * W, C, C * H * W, H * W, 1, kw["weight"], *extra, *tail, loss, plane, kept)
        _lib.call(name + "_backward", cuda, lgd, yd, B, H * W, C, C * H * W, H * W, 1, kw["weight"], *extra, *tail, 1.0, None, d, C * H * W, H * W, 1,
                  0, 0, loss2)
        got.append((loss, plane, kept, d, loss2))
    assert all(torch.equal(a, b) for a, b in zip(*got)), tag
    assert torch.equal(got[0][0], base[0]) and torch.equal(got[0][3], base[1])


@pytest.mark.parametrize("kind", MAPS[1:])
@pytest.mark.parametrize("tag", TAGS)
def test_selection_value_and_gradient_with_a_map(cuda, tag, kind):
    B, C, H, W, _, opt = PC.cases(T)[tag]
    lg, y, _ = PC.inputs(tag, T)
    md = device_map(cuda, tag, kind)
    m = md.cpu()
    v, grad, plane, kept = run(cuda, tag, md)
    mgunet.losses.check_labels(cuda)
    what = f"pixel_ce_map {tag} {kind} ({B}x{C}x{H}x{W})"
    counted = (y != PC.IGNORE).numpy()
    # the select: exact against the tie rule on the device's own weighted losses; those against float64
    want = PC.select(plane.numpy(), counted, opt["keep"], opt["min_kept"], opt["per_image"])
    assert np.array_equal(kept.numpy(), want), what
    assert not bool(np.signbit(plane.numpy()).any()) and float(plane[torch.as_tensor(~counted)].abs().sum()) == 0.0
    PC.Ref(lambda dt: {"plane": m.to(dt) * PC.pixel_losses(lg, y, opt, PC.IGNORE, dt)[0]}).check("plane", plane, PC.CAP["plane"], what)
    # value and gradient with that kept map pinned
    ref = map_reference(tag, m, kept.numpy())
    ref.check("value", v, PC.CAP["value"], what)
    ref.check("grad", grad, PC.CAP["grad"], what)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(v))
    off = torch.as_tensor(kept.numpy() != 1).to(cuda) | (md == 0)      # ignored, dropped and zero-weight pixels: exact zero rows
    if bool(off.any()):
        assert float(grad.permute(0, 2, 3, 1)[off].abs().max()) == 0.0
    if kind == "zeros":
        assert int(((md == 0) & torch.as_tensor(counted).to(cuda)).sum()) > 0
    if kind != "zeros" and C > 1 and tag not in ("equal", "equal_image"):
        assert float(grad.abs().max()) > 0.0 and not torch.equal(v, run(cuda, tag, None)[0])     # the map does change the loss


@pytest.mark.parametrize("tag", PC.LAYOUT_TAGS)
def test_layouts_with_a_map(cuda, tag):
    md = device_map(cuda, tag, "random")
    base = None
    for name in PC.LAYOUTS:
        v, grad, plane, kept = run(cuda, tag, md, name)
        if base is None:
            base = (v, grad.clone(), kept)
            ref = map_reference(tag, md.cpu(), kept.numpy())
        what = f"pixel_ce_map {tag} {name}"
        assert torch.equal(kept, base[2]), what
        ref.check("value", v, PC.CAP["value"], what)
        ref.check("grad", grad, PC.CAP["grad"], what)
        assert PC.err_of("grad", grad, base[1]) <= ref.bar("grad", PC.CAP["grad"]), what


def test_two_calls_are_bitwise_equal(cuda):
    for tag in (f"n{T + 1}", "image_of_3_weights", "equal"):
        md = device_map(cuda, tag, "random")
        a, b = run(cuda, tag, md), run(cuda, tag, md)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), tag


def count_launches(cuda, B, C, keep, backward):
    lg = torch.from_numpy(O.formula_normal("pcemap/launch/l", (B, C, 9, 11), seed=C)).to(cuda)
    y = torch.from_numpy(O.formula_labels("pcemap/launch/y", (B, 9, 11), C, seed=B)).to(cuda)
    m = torch.full((B, 9, 11), 1.5, device=cuda)
    ctx = _lib.context(cuda)
    l = lg.detach().requires_grad_(True)
    v = mgunet.pixel_cross_entropy(l, y, keep_fraction=keep, pixel_weight=m)        # scratch grown before the count
    torch.cuda.synchronize(cuda)
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        if backward:
            v.backward()
        else:
            mgunet.pixel_cross_entropy(lg, y, keep_fraction=keep, pixel_weight=m)
        torch.cuda.synchronize(cuda)
        stats = _lib.read_kernel_stats(ctx)
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)
    assert all(k["name"].startswith("pixel_ce_map") for k in stats), stats
    return sum(k["launches"] for k in stats)


@pytest.mark.parametrize("select", [False, True])
def test_launch_counts_are_those_of_the_entries_without_a_map(cuda, select):
    keep = 0.25 if select else 1.0
    for backward in (False, True):
        got = {(B, C): count_launches(cuda, B, C, keep, backward) for B in (1, 3) for C in (2, 8)}
        assert set(got.values()) == {LAUNCHES[select][int(backward)]}, (select, backward, got)


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
CFG = (3, 3, 8, 2)


def build_trainer(cuda, **kw):
    model = mgunet.UNet(*CFG)
    model.load_state_dict(O.make_unet_params(*CFG, seed=61))
    return mgunet.Trainer(model.to(cuda), comm=None, **kw)


def trainer_batch(cuda):
    """the smallest network and image of tests/test_gpu_pixel_ce.py's trainer tests; the masks are blobs of two classes, two of
    them touching, so that the labelling, the border term and the separation all have something to do"""
    x = torch.from_numpy(O.formula_normal("pcemap/tr/x", (2, 3, 32, 32), seed=62)).to(cuda)
    y = torch.zeros(2, 32, 32, dtype=torch.int64)
    y[0, 4:12, 4:12], y[0, 4:12, 12:20], y[0, 20:28, 6:14], y[1, 10:20, 10:20], y[1, 2:6, 24:30] = 1, 2, 1, 2, 1
    y[0, :2] = PC.IGNORE
    return x, y.to(cuda)


def profile_names(tr, cuda, fn):
    ctx, L = tr.model._context(cuda), _lib.lib()
    _lib.check(L.mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        out = fn()
        torch.cuda.synchronize(cuda)
        names = [k["name"] for k in _lib.read_kernel_stats(ctx)]
    finally:
        _lib.check(L.mgu_profile_enable(ctx.handle, 0), ctx.handle)
    return out, names


def test_trainer_with_border_w0_zero_is_the_trainer_without_the_arguments(cuda):
    x, y = trainer_batch(cuda)
    for kw in ({}, {"ce_weight": torch.tensor([0.5, 2.0, 1.25]), "hard_fraction": 0.5}):
        new = build_trainer(cuda, border_w0=0.0, border_sigma=3.0, border_connectivity=1, border_separate=True, **kw)
        old = build_trainer(cuda, **kw)
        assert new.border is None
        loss, names = profile_names(new, cuda, lambda: new.train_step(x, y).clone())
        assert names and not any(n.startswith("border") or n.startswith("pixel_ce_map") for n in names), names
        want = old.train_step(x, y).clone()
        assert torch.equal(loss, want) and torch.equal(new.flat, old.flat) and float(loss) > 0.0


@pytest.mark.parametrize("kw", [{}, {"ce_weight": (0.5, 2.0, 1.25)}, {"border_separate": True, "border_connectivity": 1, "hard_fraction": 0.5},
                                {"ce_weight": (0.5, 2.0, 1.25), "border_separate": True, "loss": "ce+dice"}],
                         ids=["plain", "class_weights", "separate_mined", "weights_separate_dice"])
def test_trainer_with_a_border_map_is_the_functional_composition(cuda, kw):
    x, y = trainer_batch(cuda)
    kw = dict(kw)
    kind = kw.get("loss", "ce")
    if "dice" in kind:
        y = y.clamp_min(0)
    w = torch.tensor(kw.pop("ce_weight")) if "ce_weight" in kw else None
    tr = build_trainer(cuda, border_w0=10.0, border_sigma=3.0, ce_weight=w, **kw)
    loss, names = profile_names(tr, cuda, lambda: tr.forward_backward(x, y).clone())
    assert sum(n.startswith("border_weights") for n in names) == 2 and any(n.startswith("pixel_ce_map") for n in names)
    assert not any(n.startswith("pixel_ce ") for n in names)
    # connected_components -> border_weights -> pixel_cross_entropy(pixel_weight=) on the same logits
    t2 = build_trainer(cuda)
    t2.model.train()
    logits, _, _ = t2.model(x)
    table = mgunet.connected_components(y.clamp_min(0), connectivity=kw.get("border_connectivity", 2))
    sep = kw.get("border_separate", False)
    out = mgunet.border_weights(table.labels, classes=y, class_weight=w, w0=10.0, sigma=3.0, separate=sep)
    pmap, target = out if sep else (out, y)
    l = logits.detach().requires_grad_(True)
    ce = mgunet.pixel_cross_entropy(l, target, keep_fraction=kw.get("hard_fraction", 1.0), pixel_weight=pmap)
    want = ce + mgunet.dice_loss(l, y) if "dice" in kind else ce
    assert torch.equal(loss.reshape(()), want.detach()) and float(ce.detach()) > 0.0
    if sep:
        assert int((target != y).sum()) == 2 * 8                # the two touching blobs of image 0 lose their facing columns
    assert float(pmap.max()) > 5.0                              # the gap weights are there
    # ... and so is the gradient handed to the backward pass
    want.backward()
    B, Cc, H, W = logits.shape
    ldd = (Cc + 3) // 4 * 4
    dlogits = torch.zeros((B * H * W, ldd), device=cuda)
    dlogits[:, :Cc] = l.grad.permute(0, 2, 3, 1).reshape(-1, Cc)
    _lib.call("mgu_unet_backward", cuda, dlogits, t2.grad, ctx=t2.model._context(cuda))
    if "dice" not in kind:                                      # (the trainer adds the dice rows in place: another rounding order)
        assert torch.equal(tr.grad, t2.grad)
    assert float(tr.grad.abs().max()) > 0.0
    tr.check()


def test_trainer_step_with_instances_given_is_the_step_that_labels_them(cuda):
    x, y = trainer_batch(cuda)
    kw = dict(border_w0=10.0, border_sigma=3.0, ce_weight=torch.tensor([0.5, 2.0, 1.25]), border_separate=True)
    own, given = build_trainer(cuda, **kw), build_trainer(cuda, **kw)
    table = mgunet.connected_components(y.clamp_min(0), connectivity=2)
    a = own.train_step(x, y).clone()
    b, names = profile_names(given, cuda, lambda: given.train_step(x, y, instances=table.labels).clone())
    assert torch.equal(a, b) and torch.equal(own.flat, given.flat) and float(a) > 0.0
    assert sum(n.startswith("border_weights") for n in names) == 2
    merged = build_trainer(cuda, **kw)                          # other instances, another loss: the two touching blobs as one object
    c = merged.train_step(x, y, instances=(y.clamp_min(0) != 0).to(torch.int32))
    assert not torch.equal(a, c)
