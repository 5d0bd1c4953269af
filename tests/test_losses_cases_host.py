"""The cases of tests/losses_cases.py, looked at without a GPU: every float64 reference is finite, the gradients that the GPU
tests require to be exactly zero are zero in float64, the constructed arg-max ties fall the intended way, the float64 dice
gradient equals its closed form (so the reference is not autograd agreeing with itself), and the float64 shape loss agrees with
the one-pass raw-moment restatement the kernels follow.  Under -s the cond column of the NOTES.md table is printed."""
import numpy as np
import pytest
import torch

import losses_cases as LC
import mgunet_oracle as O


def show(what, ref, cap):
    for name, cond in ref.cond.items():
        print(f"| {what} | {name} | {cond:.1e} | {ref.bar(name, cap):.1e} |")
        assert np.all(np.isfinite(ref.r64[name])), (what, name)
        assert cond < 1e-4, (what, name, cond)                  # an ill-conditioned case would make the bar meaningless


@pytest.mark.parametrize("shape", LC.TV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tv_cases(shape):
    ref = LC.tv_reference(shape)
    show(f"tv {shape}", ref, LC.CAP["tv"])
    assert ref.r64["dx"].any() and LC.FLOOR < ref.bar("dx", LC.CAP["tv"]) <= LC.CAP["tv"]
    if shape == LC.TV_CHAINED:
        chained = LC.tv_reference(shape, True)
        show(f"tv {shape} chained", chained, LC.CAP["tv"])
        v = float(ref.r64["value"])
        assert np.allclose(chained.r64["dx"], ref.r64["dx"] * (LC.TV_UP + v) / LC.TV_UP, rtol=1e-12, atol=0)
    if shape == LC.TV_BIG:
        assert int(np.prod(shape)) > 1024 * 1024
    x = LC.tv_input(shape)
    for name in LC.tv_layouts(shape):                            # every layout holds the same logical values, and is what it says
        v = LC.TV_LAYOUTS[name](x)
        assert torch.equal(v, x) and tuple(v.shape) == tuple(shape)
        if name == "nhwc" and shape[1] > 1:                      # (the stride of a one-element dimension says nothing)
            assert v.stride(1) == 1
        if name == "chslice":
            assert v.stride(1) == 1 and v.stride(3) == shape[1] + 2 and v.storage_offset() == 1
        if name == "crop":
            assert v.stride(2) == shape[3] + 5 and v.stride(3) == 1 and not v.is_contiguous()


@pytest.mark.parametrize("tag", list(LC.DICE_CASES))
def test_dice_cases(tag):
    B, C, H, W, scale, smooth = LC.DICE_CASES[tag]
    lg, y, _ = LC.dice_inputs(tag)
    ref = LC.dice_reference(tag)
    show(f"dice {tag}", ref, LC.CAP["dice"])
    assert int(y.min()) >= 0 and int(y.max()) < C
    if C == 1:
        assert not ref.r64["dlogits"].any() and float(ref.r64["value"]) == 0.0
    else:
        assert ref.r64["dlogits"].any()
    if tag == "cap":
        assert H * W > 128 * 1024
    if tag == "absent":
        assert not (y == 2).any() and not (y[1] == 3).any() and (y[0] == 3).any() and (y[2] == 3).any()
    if tag == "saturated":                                       # most pixels are one-hot to fp32 precision
        assert float((torch.softmax(lg, 1).max(1).values > 1 - 1e-6).float().mean()) > 0.5
    if tag in LC.DICE_RAW:
        raw = LC.dice_raw_reference(tag)
        show(f"dice accumulate {tag}", raw, LC.CAP["dice"])
        inc = np.abs(ref.r64["dlogits"]).max() * LC.DICE_RAW_SCALE * LC.DICE_RAW_SCALE_DEV
        assert 0.1 < inc / (3 * LC.DICE_RAW_PREFILL) < 10, inc  # increment and prefill of one magnitude: a wrong increment shows
    x = lg[:, :, :6, :7]
    for name, lay in LC.DICE_LAYOUTS.items():
        assert torch.equal(lay(x), x), name


@pytest.mark.parametrize("tag", ["c5", "c8", "absent"])
def test_dice_float64_gradient_is_the_closed_form(tag):
    lg, y, smooth = LC.dice_inputs(tag)
    ref = LC.dice_reference(tag)
    got = LC.dice_closed_form(lg, y, smooth).numpy()
    assert np.abs(got - ref.r64["dlogits"]).max() <= 1e-12 * np.abs(ref.r64["dlogits"]).max()


@pytest.mark.parametrize("tag", list(LC.FEATCONS_CASES))
def test_feature_consistency_cases(tag):
    B, N, D, mrule, yrule, coin, needs = LC.FEATCONS_CASES[tag]
    fu, fg, y, margin, _ = LC.featcons_inputs(tag)
    ref = LC.featcons_reference(tag)
    show(f"feature consistency {tag}", ref, LC.CAP["featcons"])
    assert ("dfu" in ref.r64) == needs[0] and ("dfg" in ref.r64) == needs[1]
    dist = LC.featcons_distances(fu, fg)
    grads = [ref.r64[k].reshape(B, N, D) for k in ("dfu", "dfg") if k in ref.r64]
    if coin is not None:                                         # a coincident row has a zero gradient whatever its y
        assert torch.equal(fu[0, 0], fg[0, 0]) and float(y[0, 0]) == coin and abs(float(dist[0, 0]) - 1e-4) < 1e-12
        assert all(not g[0, 0].any() for g in grads)
    if mrule == "below":                                         # the hinge is off everywhere: rows with y = 0 have no gradient
        assert margin < float(dist.min()) and (y == 0).any() and (y == 1).any()
        assert all(not g[(y == 0).numpy()].any() and g[(y == 1).numpy()].any() for g in grads)
    elif mrule == "above":
        assert margin > float(dist.max())
        assert all(np.abs(g).reshape(B * N, D).max(1).min() > 0 for g in grads)
    elif B * N >= 100 and yrule == "hard":                       # both branches carry weight
        hinge = ((dist < margin) & (y == 0)).double().mean()
        assert 0.05 < float(hinge) < 0.6 and 0.2 <= float((y == 1).double().mean()) <= 0.8, (float(hinge), y.mean())
    if N == 1:                                                   # a lone row's hinge is no cancellation
        assert abs(margin - float(dist[0, 0])) > 0.05
    if yrule == "soft":
        assert sorted(round(float(v), 6) for v in np.unique(y.numpy())) == [0.2, 0.5]
    if tag == "cap":
        assert B * N > 65536


def test_shape_mask_cases_and_raw_moment_restatement():
    masks = LC.shape_masks()
    assert masks.shape == (LC.SHAPE_COUNT, LC.SHAPE_HW, LC.SHAPE_HW) and LC.SHAPE_COUNT > 64
    first = LC.SHAPE_COUNT - len(LC.SHAPE_SPECIAL)
    special = dict(zip(LC.SHAPE_SPECIAL, masks[first:]))
    assert first < 64 <= first + LC.SHAPE_SPECIAL.index("px9")  # both sides of the 10-pixel threshold sit in the second workgroup
    count = {k: int(m.sum()) for k, m in special.items()}
    assert count == {"full": 576, "borders": 176, "px9": 9, "px10": 10, "row12": 12, "diag12": 12, "diag13": 13, "empty": 0}
    b = special["borders"]
    assert b[0].all() and b[-1].all() and b[:, 0].all() and b[:, -1].all() and not b[2:-2, 2:-2].any()
    assert all(int(m.sum()) >= 10 for m in masks[:first])
    assert len({m.tobytes() for m in masks}) == LC.SHAPE_COUNT                  # 70 different objects
    # each object on its own, then the two calls: float64 oracle == one-pass raw moments to 1e-8
    worst = 0.0
    for i, m in enumerate(masks):
        raw = LC.shape_term_raw_moments(m)
        ref = O._ellipse_object_term(torch.from_numpy(m), LC.SHAPE_EPS, torch.float64)
        assert (raw is None) == (ref is None) == (int(m.sum()) < 10), i
        if raw is not None:
            assert np.isfinite(raw) and abs(raw - float(ref)) <= 1e-8 * max(1.0, abs(float(ref))), (i, raw, float(ref))
            worst = max(worst, abs(raw - float(ref)) / max(1.0, abs(float(ref))))
    ref, raw = LC.shape_reference(masks), LC.shape_loss_raw_moments(masks)
    assert abs(ref - raw) <= 1e-8 * max(1.0, abs(ref))
    # dropping the 10-pixel object, or keeping the 9-pixel one, moves the loss by far more than the bar
    kept = [m for k, m in enumerate(masks) if k != first + LC.SHAPE_SPECIAL.index("px10")]
    assert abs(LC.shape_reference(kept) - ref) > 100 * LC.SHAPE_BAR * abs(ref)
    big = LC.shape_big_masks()
    assert big.shape == (2, LC.SHAPE_BIG_HW, LC.SHAPE_BIG_HW) and LC.SHAPE_BIG_HW ** 2 > 256 * 1024
    assert big[1][:, 0].any() and big[1][:, -1].any() and 1000 < big[1].sum() < 2000 and big[0].sum() > 50000
    rb, wb = LC.shape_reference(big), LC.shape_loss_raw_moments(big)
    assert abs(rb - wb) <= 1e-8 * max(1.0, abs(rb))
    # the fp32 route is no yardstick for the thin objects
    d32 = abs(float(O._ellipse_object_term(torch.from_numpy(special["diag12"]), LC.SHAPE_EPS)) -
              float(O._ellipse_object_term(torch.from_numpy(special["diag12"]), LC.SHAPE_EPS, torch.float64)))
    print(f"shape: 24 x 24 call {ref:.9f}, 520 x 520 call {rb:.9f}, worst |oracle64 - raw moments| {worst:.1e}, "
          f"fp32 oracle off by {d32:.2g} on the 12-pixel diagonal")


@pytest.mark.parametrize("C", LC.PROBS_CLASSES)
def test_shape_probability_cases_and_ties(C):
    p = LC.probs_input(C)
    assert p.dtype == torch.float32 and tuple(p.shape) == (LC.PROBS_B, C, LC.PROBS_H, LC.PROBS_W)
    lab = torch.argmax(p, dim=1)
    t01 = p[0][:, LC.TIE_01[0], LC.TIE_01[1]]
    assert torch.equal(t01[0], t01[1]) and (t01[0] == p[0][:, LC.TIE_01[0], LC.TIE_01[1]].max(0).values).all()
    assert (lab[0][LC.TIE_01] == 0).all()                        # first maximum: class 0, not foreground
    fg = [int((lab[b] == 1).sum()) for b in range(LC.PROBS_B)]
    assert fg[1] == 7 and fg[0] >= 10 and fg[2] >= 10            # image 1 is skipped and leaves the denominator
    ref = LC.probs_reference(p)
    assert np.isfinite(ref) and ref > 0

    def with_labels(edit):
        l2 = lab.clone()
        edit(l2)
        return float(O.elliptical_shape_loss(None, [[l2[b] == 1 for b in range(LC.PROBS_B)]], LC.SHAPE_EPS, dtype=torch.float64))

    assert with_labels(lambda l: None) == ref
    # either tie read the other way, or image 1 counted, moves the loss by far more than the bar
    assert abs(with_labels(lambda l: l[0].__setitem__(LC.TIE_01, 1)) - ref) > 1e-3 * ref
    both = 0.5 * (float(O._ellipse_object_term(lab[0] == 1, LC.SHAPE_EPS, torch.float64)) +
                  float(O._ellipse_object_term(lab[2] == 1, LC.SHAPE_EPS, torch.float64)))
    assert abs(both - ref) <= 1e-12 * ref and abs(both * 2 / 3 - ref) > 1e-3 * ref
    if C >= 3:
        t12 = p[0][:, LC.TIE_12[0], LC.TIE_12[1]]
        assert torch.equal(t12[1], t12[2]) and (t12[1] == t12.max(0).values).all()
        assert (lab[0][LC.TIE_12] == 1).all()                    # first maximum: class 1, foreground
        assert abs(with_labels(lambda l: l[0].__setitem__(LC.TIE_12, 2)) - ref) > 1e-3 * ref
        assert (lab >= 2).any()


def test_resize_and_gather_cases():
    for src, dst in LC.RESIZE_SIZES:
        for C in LC.RESIZE_CHANNELS:
            ref = LC.resize_reference(src, dst, C)
            show(f"resize {src} -> {dst} C = {C}", ref, LC.CAP["resize"])
            assert ref.r64["map"].shape == (LC.RESIZE_B, C) + dst and LC.RESIZE_OFF + C <= LC.RESIZE_LD
    for D in LC.GATHER_DIMS:
        table, ids = LC.gather_inputs(D)
        ref = LC.gather_reference(table, ids)
        flat, rows = ids.reshape(-1), ref.reshape(-1, D)
        for want in LC.GATHER_PLANTED:
            assert (flat == want).any()
        for i, r in zip(flat.tolist(), rows):
            assert torch.equal(r, table[i]) if 0 <= i < LC.GATHER_R else not r.any()
        assert table.abs().min() > 0 and LC.GATHER_OFF + D < LC.GATHER_LD
