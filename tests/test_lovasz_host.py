"""The float64 reference of the Lovasz-Softmax loss (tests/lovasz_cases.py) against the definition it stands for, and the host side
of the feature: the reference equals the brute-force Lovasz extension of the Jaccard set function, hard errors give 1 - IoU,
hand-computed tiny cases for per_image / classes / ignore_index, the closed form of the all-equal case, why the closed-form gradient
exists (the differenced fp32 formulation at 2^21 pixels), and the names the feature adds.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import lovasz_cases as LV
import mgunet

T = 4096      # any tile size serves the host checks: the cases only size themselves by it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def from_probs(p1):
    """two-class logits (1, 2, 1, n) whose softmax gives class 1 the probabilities p1"""
    p1 = torch.tensor(p1, dtype=torch.float64)
    return torch.stack([torch.log(1.0 - p1), torch.log(p1)])[None, :, None, :]


def segment_loss(errors, fg):
    """sum e_(k) g_k by the closed forms, along the tie rule's order"""
    e, fg = np.asarray(errors, dtype=np.float64), np.asarray(fg, dtype=bool)
    order = np.argsort(-e, kind="stable")
    return float((e[order] * LV.jaccard_increments(fg[order])).sum())


def test_closed_forms_equal_the_bruteforce_lovasz_extension():
    """every N <= 7, random foreground masks and every mask of N <= 4 (G = 0 and G = N included), errors with ties"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for n in range(1, 8):
        masks = list(itertools.product((False, True), repeat=n)) if n <= 4 else \
            [np.zeros(n, bool), np.ones(n, bool)] + [rng.random(n) < q for q in (0.1, 0.3, 0.5, 0.7, 0.9) for _ in range(4)]
        for fg in masks:
            for tied in (False, True):
                e = rng.random(n)
                if tied:
                    e = np.round(e * 3) / 3
                brute, closed = LV.lovasz_extension_bruteforce(e, fg), segment_loss(e, fg)
                worst = max(worst, abs(brute - closed))
                # the increments themselves, not only their weighted sum
                order = np.argsort(-e, kind="stable")
                wrong, before, inc = np.zeros(n, bool), 0.0, []
                for i in order:
                    wrong[i] = True
                    now = LV.jaccard_loss_of_set(fg, wrong)
                    inc.append(now - before)
                    before = now
                assert np.abs(np.array(inc) - LV.jaccard_increments(np.asarray(fg)[order])).max() <= 1e-15
    print(f"closed form against the set function: worst |difference| {worst:.1e}")
    assert worst <= 1e-15


def test_reference_is_the_extension_per_class():
    lg, y, _, _ = LV.inputs("ignore", T)
    B, C = lg.shape[:2]
    e = LV.softmax_errors(lg, y).numpy().reshape(C, -1)
    yy = y.reshape(-1).numpy()
    keep = yy != LV.IGNORE
    terms = [LV.lovasz_extension_bruteforce(e[c][keep], (yy == c)[keep]) for c in range(C)]
    assert abs(float(LV.lovasz_reference(lg, y)) - sum(terms) / C) <= 1e-14


def test_hard_errors_give_one_minus_iou():
    rng = np.random.default_rng(5)
    for n in (1, 2, 9, 300):
        for _ in range(6):
            fg, pred = rng.random(n) < 0.4, rng.random(n) < 0.4
            e = (fg != pred).astype(np.float64)
            union = int((fg | pred).sum())
            iou_loss = 1.0 - int((fg & pred).sum()) / union if union else 0.0
            assert abs(segment_loss(e, fg) - iou_loss) <= 1e-14
    # through the reference: saturated logits, mean over the present classes of 1 - IoU of the arg-max map
    lg, y, _, _ = LV.inputs("saturated", T)
    pred = lg.argmax(1)
    ious = [1.0 - float(((pred == c) & (y == c)).sum()) / float(((pred == c) | (y == c)).sum()) for c in range(lg.shape[1]) if bool((y == c).any())]
    assert abs(float(LV.lovasz_reference(lg, y)) - sum(ious) / len(ious)) <= 1e-14


# p(class 1) of four pixels: image 0 = pixels 0, 1; image 1 = pixels 2, 3 (class 1 absent from image 1)
P1 = [0.8, 0.4, 0.3, 0.6]
Y = [1, 0, 0, 0]


def tiny(y=Y, **kw):
    lg = from_probs(P1)[0, :, 0, :].reshape(2, 2, 2).permute(1, 0, 2)[:, :, None, :].contiguous()   # (B = 2, C = 2, H = 1, W = 2)
    return float(LV.lovasz_reference(lg, torch.tensor(y).reshape(2, 1, 2), **kw))


def test_hand_computed_tiny_cases():
    # over the batch.  class 1 (G = 1): errors .2 (fg) .4 .3 .6 -> order 3, 1, 2, 0: g = 1/2, 1/6, 1/12, 1/4
    #                  class 0 (G = 3): errors .2 (bg) .4 .3 .6 -> order 3, 1, 2, 0: g = 1/3, 1/3, 1/3, 0
    c1, c0 = 0.6 / 2 + 0.4 / 6 + 0.3 / 12 + 0.2 / 4, (0.6 + 0.4 + 0.3) / 3
    assert abs(tiny() - (c1 + c0) / 2) <= 1e-15
    assert abs(tiny(classes="all") - (c1 + c0) / 2) <= 1e-15
    # per image.  image 0: class 1 order 1 (bg), 0 (fg): g = 1/2, 1/2; class 0 order 1 (fg), 0 (bg): g = 1, 0
    #             image 1: class 0 both foreground: g = 1/2, 1/2; class 1 absent: skipped, or ("all") g = 1 on its largest error
    im0, im1_c0, im1_c1 = ((0.4 + 0.2) / 2 + 0.4) / 2, (0.6 + 0.3) / 2, 0.6
    assert abs(tiny(per_image=True) - (im0 + im1_c0) / 2) <= 1e-15
    assert abs(tiny(per_image=True, classes="all") - (im0 + (im1_c0 + im1_c1) / 2) / 2) <= 1e-15
    # pixel 3 ignored, over the batch.  class 1: order 1, 2, 0: g = 1/2, 1/6, 1/3; class 0 (G = 2): order 1, 2, 0: g = 1/2, 1/2, 0
    ig = [1, 0, 0, LV.IGNORE]
    assert abs(tiny(ig) - ((0.4 / 2 + 0.3 / 6 + 0.2 / 3) + (0.4 + 0.3) / 2) / 2) <= 1e-15
    # image 1 ignored as a whole, per image: it adds 0 and still counts in the mean over images
    assert abs(tiny([1, 0, LV.IGNORE, LV.IGNORE], per_image=True) - im0 / 2) <= 1e-15
    assert tiny([LV.IGNORE] * 4) == 0.0 and tiny([LV.IGNORE] * 4, per_image=True, classes="all") == 0.0
    # another ignore_index
    assert abs(tiny([1, 0, 0, 7], ignore_index=7) - tiny(ig)) <= 1e-15


def test_ignored_pixels_get_no_gradient_and_pinned_ranks_reproduce_the_sort():
    lg, y, classes, per_image = LV.inputs("ignore_image", T)
    l = lg.double().requires_grad_(True)
    v = LV.lovasz_reference(l, y, classes, per_image)
    v.backward()
    assert float(l.grad.permute(0, 2, 3, 1)[y == LV.IGNORE].abs().max()) == 0.0 and float(l.grad.abs().max()) > 0.0
    # ranks built on the host by the tie rule, handed back as `ranks`: the same value
    e = LV.softmax_errors(lg, y).numpy()
    B, C = lg.shape[:2]
    ranks = np.full(e.shape, -1, dtype=np.int32)
    for b in range(B):
        keep = np.nonzero(y[b].reshape(-1).numpy() != LV.IGNORE)[0]
        for c in range(C):
            order = np.argsort(-e[c, b].reshape(-1)[keep], kind="stable")
            ranks[c, b].reshape(-1)[keep[order]] = np.arange(len(keep))
    assert LV.check_ranks(e, ranks, y.numpy(), per_image) == 0
    assert float(LV.lovasz_reference(lg, y, classes, per_image, ranks=ranks)) == float(v.detach())


def test_all_logits_equal_closed_form():
    """one tie over the whole segment: p = 1 / C everywhere, the foreground's error 1 - 1 / C comes first and takes g = 1 / G each,
    the background gets 0: every present class contributes 1 - 1 / C.  For C = 2 every error is 1 / 2 and sum g = 1."""
    for tag, C in (("equal_c2", 2), ("equal_c3", 3)):
        lg, y, classes, per_image = LV.inputs(tag, T)
        assert abs(float(LV.lovasz_reference(lg, y, classes, per_image)) - (1.0 - 1.0 / C)) <= 1e-14


def test_degenerate_cases_of_the_reference():
    for tag in ("c1", "all_ignored", "all_ignored_all"):
        lg, y, classes, per_image = LV.inputs(tag, T)
        r = LV.reference(tag, T)
        assert float(r.r64["value"]) == 0.0 and float(np.abs(r.r64["grad"]).max()) == 0.0


def test_case_table_covers_the_sizes_and_edges():
    cs = LV.cases(T)
    sizes = {B * H * W for (B, C, H, W, kind, _, per_image) in cs.values() if kind == "random"}
    assert sizes == {1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5}
    assert {c[1] for c in cs.values()} >= {1, 2, 3, 5, 8}
    assert max(c[0] * c[2] * c[3] for c in cs.values()) <= 65536
    lg, y, _, _ = LV.inputs("image_present_64", T)
    assert not bool((y[1] == 2).any()) and bool((y[2] == LV.IGNORE).all()) and bool((y[0] == 2).any())
    # exact errors of the two digit cases, as far as the host can tell (the GPU test looks at the device's own bits)
    lg, y, _, _ = LV.inputs("high_digit", T)
    bits = LV.softmax_errors(lg, y, torch.float32).numpy().view(np.uint32)
    assert (bits & 0xFFFFF == 0).all() and len(np.unique(bits >> 20)) >= 4
    lg, y, _, _ = LV.inputs("low_digit", T)
    e64 = LV.softmax_errors(lg, y).numpy()
    assert np.abs(e64 - 0.75).max() < 2.0 ** -13
    lg, y, _, _ = LV.inputs("saturated", T)
    assert set(np.unique(LV.softmax_errors(lg, y, torch.float32).numpy())) == {0.0, 1.0}


def test_differenced_fp32_formulation_misses_the_kernel_bar():
    """Why the gradient is a closed form: at N = 2^21 (10 % foreground, uniform errors) the published fp32 formulation --
    jaccard = 1 - inter / union, neighbours differenced -- is off from float64 by far more than any bar the kernel is held to
    (CAP["grad"] bounds every one of them), while the closed forms evaluated in fp32 stay inside it."""
    n = 1 << 21
    rng = np.random.default_rng(2021)
    fg = rng.random(n) < 0.1
    e = rng.random(n)
    order = np.argsort(-e, kind="stable")
    g64 = LV.jaccard_increments(fg[order])
    diff = LV.differenced_fp32_gradient(e[order], fg[order]).astype(np.float64)
    worst = float(np.abs(diff - g64).max() / g64.max())
    med = float(np.median(np.abs(diff - g64)) / np.median(g64))
    closed32 = float(np.abs(g64.astype(np.float32).astype(np.float64) - g64).max() / g64.max())
    print(f"differenced fp32 at 2^21: worst {worst:.1e} of the largest, median error {med:.1e} of the median; closed form rounded: {closed32:.1e}")
    assert worst > LV.CAP["grad"] and med > 0.01
    assert closed32 <= LV.FLOOR
    # the value does not suffer
    v64 = float((e[order] * g64).sum())
    assert abs(float((e[order].astype(np.float32) * diff.astype(np.float32)).sum(dtype=np.float64)) - v64) <= 1e-6 * v64


def test_names_are_exported_and_declared():
    assert "lovasz_softmax" in mgunet.__all__ and callable(mgunet.lovasz_softmax)
    assert callable(mgunet.losses._lovasz_debug)
    header = open(os.path.join(ROOT, "include", "mgunet.h")).read()
    for name in ("mgu_lovasz_softmax", "mgu_lovasz_softmax_backward", "mgu_lovasz_tile"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    protos = mgunet._lib.parse_header()
    assert protos["mgu_lovasz_softmax"][2] and protos["mgu_lovasz_softmax_backward"][2] and not protos["mgu_lovasz_tile"][2]
    assert "lovasz.hip" in open(os.path.join(ROOT, "mingraph-unet_amd", "csrc", "Makefile")).read()


def test_trainer_rejects_an_unknown_loss_naming_the_four():
    class NoModel:
        def named_parameters(self):
            raise AssertionError("the loss name is checked before the model is touched")

    with pytest.raises(ValueError) as ei:
        mgunet.Trainer(NoModel(), loss="lovasz+ce")
    for name in ("'ce'", "'ce+dice'", "'ce+lovasz'", "'ce+dice+lovasz'"):
        assert name in str(ei.value), str(ei.value)
    with pytest.raises(ValueError, match="lovasz_classes"):
        mgunet.Trainer(NoModel(), loss="ce+lovasz", lovasz_classes="some")
