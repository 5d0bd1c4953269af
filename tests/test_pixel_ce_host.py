"""The float64 reference of the pixel cross-entropy (tests/pixel_ce_cases.py) against what it stands for, and the host side of the
feature: the reference equals F.cross_entropy in float64 for every (weight, label_smoothing, ignore) combination without mining,
the focal term at gamma = 0 and by hand, the selection oracle against a brute-force sort, K at its edges, the names the feature
adds, the argument refusals, class_weights against hand values, and six wrong readings of the definition that the cases tell apart.
No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mgunet
import pixel_ce_cases as PC

T = 4096      # any tile size serves the host checks: the cases only size themselves by it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("ignore", [False, True])
def test_reference_is_torch_cross_entropy_without_mining(weighted, eps, ignore):
    lg, y, _ = PC.inputs("c4", T)
    if not ignore:
        y = y.clamp_min(0)
    assert bool((y == PC.IGNORE).any()) == ignore
    opt = PC.options(weight=PC.W4 if weighted else None, eps=eps)
    w = torch.tensor(PC.W4, dtype=torch.float64) if weighted else None
    want = F.cross_entropy(lg.double(), y, weight=w, label_smoothing=eps, ignore_index=PC.IGNORE)
    got = PC.pixel_ce_reference(lg, y, opt)
    assert abs(float(got) - float(want)) <= 1e-14
    # the per-pixel losses are torch's reduction="none"
    per = F.cross_entropy(lg.double(), y, weight=w, label_smoothing=eps, ignore_index=PC.IGNORE, reduction="none")
    assert float((PC.pixel_losses(lg, y, opt)[0] - per).abs().max()) <= 1e-14
    # and so is the gradient
    a, b = lg.double().requires_grad_(True), lg.double().requires_grad_(True)
    PC.pixel_ce_reference(a, y, opt).backward()
    F.cross_entropy(b, y, weight=w, label_smoothing=eps, ignore_index=PC.IGNORE).backward()
    assert float((a.grad - b.grad).abs().max()) <= 1e-15


def test_focal_term():
    lg, y, _ = PC.inputs("c4", T)
    # (1 - p)^0 = 1: the focal form at gamma 0 is the weighted cross-entropy (the options refuse 0 < gamma < 1, the formula does not)
    l0 = PC.pixel_losses(lg, y, PC.options(weight=PC.W4))[0]
    p = torch.softmax(lg.double(), 1)
    ys = y.clamp_min(0)
    py = p.gather(1, ys[:, None])[:, 0]
    w = torch.tensor(PC.W4, dtype=torch.float64)[ys]
    focal0 = torch.where(y == PC.IGNORE, torch.zeros_like(py), w * (1.0 - py) ** 0.0 * -torch.log(py))
    assert float((focal0 - l0).abs().max()) <= 1e-14
    # two pixels by hand: p_y = 0.8 and 0.25, gamma 2, weights (2, 0.5)
    lg2 = torch.log(torch.tensor([[0.8, 0.75], [0.2, 0.25]], dtype=torch.float64))[None, :, None, :]      # (1, 2, 1, 2)
    y2 = torch.tensor([[[0, 1]]])
    opt = PC.options(weight=(2.0, 0.5), gamma=2.0)
    l = PC.pixel_losses(lg2, y2, opt)[0].reshape(-1)
    hand = [2.0 * 0.2 ** 2 * -math.log(0.8), 0.5 * 0.75 ** 2 * -math.log(0.25)]
    assert abs(float(l[0]) - hand[0]) <= 1e-15 and abs(float(l[1]) - hand[1]) <= 1e-15
    assert abs(float(PC.pixel_ce_reference(lg2, y2, opt)) - sum(hand) / 2.5) <= 1e-15
    # keeping one of the two: the larger loss alone over its own weight
    assert abs(float(PC.pixel_ce_reference(lg2, y2, PC.options(weight=(2.0, 0.5), gamma=2.0, keep=0.5))) - hand[1] / 0.5) <= 1e-15


def test_selection_oracle_is_the_bruteforce_sort():
    rng = np.random.default_rng(3)
    for B, H, W in ((1, 1, 1), (1, 1, 7), (3, 4, 5), (2, 9, 11)):
        for per_image in (False, True):
            for keep, min_kept in ((0.25, 0), (1.0 / 3.0, 2), (0.5, 1000), (1.0, 0), (1e-9, 0)):
                loss = (np.round(rng.random((B, H, W)) * 6) / 6).astype(np.float32)       # many ties
                counted = rng.random((B, H, W)) < 0.8
                if B == 3:
                    counted[1] = False
                a = PC.select(loss, counted, keep, min_kept, per_image)
                b = PC.select_bruteforce(loss, counted, keep, min_kept, per_image)
                assert np.array_equal(a, b), (B, H, W, per_image, keep, min_kept)
                assert ((a == -1) == ~counted).all()
    # ties go to the lower index
    loss = np.array([[[1.0, 2.0, 1.0, 1.0, 0.5]]], dtype=np.float32)
    assert PC.select(loss, np.ones_like(loss, bool), 0.6, 0, False).reshape(-1).tolist() == [1, 1, 1, 0, 0]
    assert PC.select(loss, np.ones_like(loss, bool), 0.6, 0, False, "ties_high").reshape(-1).tolist() == [0, 1, 1, 1, 0]


def test_kept_count_at_its_edges():
    want = {   # (n, f) -> ceil(f n) by hand
        (0, 0.25): 0, (1, 0.25): 1, (3, 0.25): 1, (4097, 0.25): 1025,
        (0, 1.0 / 3.0): 0, (1, 1.0 / 3.0): 1, (3, 1.0 / 3.0): 1, (4097, 1.0 / 3.0): 1366,
        (0, 1.0): 0, (1, 1.0): 1, (3, 1.0): 3, (4097, 1.0): 4097}
    for (n, f), byf in want.items():
        assert int(np.ceil(np.float64(f) * np.float64(n))) == byf
        for min_kept in (0, max(byf - 1, 0), byf + 1 if byf < n else n, n + 5):      # below, between and above
            K = PC.kept_count(n, f, min_kept)
            assert K == min(n, max(min_kept, byf)), (n, f, min_kept)
            assert 0 <= K <= n and (K >= min(n, min_kept))
    assert PC.kept_count(3, 1.0 / 3.0, 0) == 1 and PC.kept_count(3, 1.0 / 3.0, 2) == 2 and PC.kept_count(3, 1.0 / 3.0, 9) == 3


def test_names_are_exported_and_declared():
    for name in ("pixel_cross_entropy", "class_weights"):
        assert name in mgunet.__all__ and callable(getattr(mgunet, name)), name
    assert callable(mgunet.losses._pixel_ce_debug)
    header = open(os.path.join(ROOT, "include", "mgunet.h")).read()
    for name in ("mgu_pixel_ce", "mgu_pixel_ce_backward", "mgu_pixel_ce_tile"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    protos = mgunet._lib.parse_header()
    assert protos["mgu_pixel_ce"][2] and protos["mgu_pixel_ce_backward"][2] and not protos["mgu_pixel_ce_tile"][2]
    assert len(protos["mgu_pixel_ce"][1]) == 20 and len(protos["mgu_pixel_ce_backward"][1]) == 26      # context and stream included
    import ctypes
    assert protos["mgu_pixel_ce"][1][12] is ctypes.c_double and protos["mgu_pixel_ce"][1][13] is ctypes.c_int64
    assert "pixel_ce.hip" in open(os.path.join(ROOT, "mingraph-unet_amd", "csrc", "Makefile")).read()


class NoModel:
    def named_parameters(self):
        raise AssertionError("the loss options are checked before the model is touched")


@pytest.mark.parametrize("kw, match", [
    ({"label_smoothing": 1.0}, "label_smoothing"), ({"label_smoothing": -0.1}, "label_smoothing"),
    ({"focal_gamma": 0.5}, "focal_gamma"), ({"focal_gamma": -1.0}, "focal_gamma"),
    ({"focal_gamma": 2.0, "label_smoothing": 0.1}, "label_smoothing"),
    ({"hard_fraction": 0.0}, "keep_fraction"), ({"hard_fraction": 1.5}, "keep_fraction"), ({"hard_min_kept": -1}, "min_kept"),
    ({"ce_weight": torch.tensor([1.0, -1.0])}, "weights"), ({"ce_weight": [1.0, 2.0]}, "weight")])
def test_trainer_refuses_bad_options_before_touching_the_model(kw, match):
    with pytest.raises(ValueError, match=match):
        mgunet.Trainer(NoModel(), **kw)


def test_trainer_still_names_its_losses():
    with pytest.raises(ValueError) as ei:
        mgunet.Trainer(NoModel(), loss="focal")
    for name in ("'ce'", "'ce+dice'", "'ce+lovasz'", "'ce+dice+lovasz'"):
        assert name in str(ei.value)
    assert mgunet.engine.LOSSES == ("ce", "ce+dice", "ce+lovasz", "ce+dice+lovasz")


def test_function_refuses_cpu_tensors_and_bad_shapes():
    lg, y = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HIP device"):
        mgunet.pixel_cross_entropy(lg, y)
    from mgunet.losses import pixel_ce_options
    for kw, match in (({"label_smoothing": 1.0}, "label_smoothing"), ({"focal_gamma": 0.99}, "focal_gamma"),
                      ({"keep_fraction": 0.0}, "keep_fraction"), ({"keep_fraction": float("nan")}, "keep_fraction"),
                      ({"min_kept": -3}, "min_kept"), ({"focal_gamma": 1.0, "label_smoothing": 0.5}, "label_smoothing")):
        args = {"weight": None, "label_smoothing": 0.0, "focal_gamma": 0.0, "keep_fraction": 1.0, "min_kept": 0, "per_image": False}
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            pixel_ce_options(**args)
    with pytest.raises(ValueError, match="num_classes"):
        pixel_ce_options(torch.ones(3), 0.0, 0.0, 1.0, 0, False, num_classes=2)
    assert pixel_ce_options(None, 0.0, 0.0, 1.0, 0, False) == (0.0, 0.0, 1.0, 0, 0)
    assert pixel_ce_options(torch.ones(2), 0.1, 0.0, 0.25, 7, True, 2) == (0.1, 0.0, 0.25, 7, 1)


def test_class_weights_against_hand_values():
    counts = [600, 300, 0, 100]                                # f = .6 .3 - .1: median of the three that occur = .3
    w = mgunet.class_weights(counts)
    assert w.dtype == torch.float32 and tuple(w.shape) == (4,)
    assert np.allclose(w.numpy(), [0.5, 1.0, 0.0, 3.0], rtol=1e-7, atol=0)
    assert np.allclose(mgunet.class_weights(counts, "inverse").numpy(), [1 / 1.8, 1 / 0.9, 0.0, 1 / 0.3], rtol=1e-7, atol=0)
    assert np.allclose(mgunet.class_weights(counts, "enet").numpy(),
                       [1 / math.log(1.62), 1 / math.log(1.32), 0.0, 1 / math.log(1.12)], rtol=1e-7, atol=0)
    assert np.allclose(mgunet.class_weights([30, 10]).numpy(), [0.5 / 0.75, 0.5 / 0.25], rtol=1e-7, atol=0)      # even count: mean of the two
    assert mgunet.class_weights(torch.zeros(3)).tolist() == [0.0, 0.0, 0.0]
    conf = torch.tensor([[5, 1], [2, 2]])
    assert np.allclose(mgunet.class_weights(conf.sum(1)).numpy(), [0.5 / 0.6, 0.5 / 0.4], rtol=1e-7, atol=0)
    with pytest.raises(ValueError, match="median_frequency"):
        mgunet.class_weights(counts, "balanced")
    with pytest.raises(ValueError):
        mgunet.class_weights([1, -1])


def test_case_table_covers_the_sizes_and_edges():
    cs = PC.cases(T)
    sizes = {B * H * W for (B, C, H, W, kind, opt) in cs.values() if kind == "random" and opt["keep"] > 1e-6}
    assert sizes == {1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 17}
    assert {c[1] for c in cs.values()} >= set(range(1, 9))
    assert max(c[0] * c[2] * c[3] for c in cs.values()) <= 16384
    lg, y, opt = PC.inputs("image_of_3", T)
    assert bool((y[2] == PC.IGNORE).all()) and not bool((y[:2] == PC.IGNORE).any()) and opt["per_image"]
    # the key edges, as far as the host can tell in fp32 (the GPU test looks at the device's own bits)
    lg, y, opt = PC.inputs("equal", T)
    l = PC.pixel_losses(lg, y, opt)[0]
    assert float((l - math.log(2.0)).abs().max()) <= 1e-15 and 1 < PC.kept_count(l.numel(), opt["keep"], opt["min_kept"]) < l.numel()
    lg, y, opt = PC.inputs("straddle", T)
    l = PC.pixel_losses(lg, y, opt)[0].reshape(-1)
    tie = (l - math.log(2.0)).abs() <= 1e-15
    assert int(tie.sum()) == sum(PC.STRADDLE_TIE) and bool(tie[T - PC.STRADDLE_TIE[0]:T + PC.STRADDLE_TIE[1]].all())
    assert int((l > 1.0).sum()) == PC.STRADDLE_HARD and int((l[:T] > 1.0).sum()) == PC.STRADDLE_HARD
    r = PC.kept_count(l.numel(), opt["keep"], opt["min_kept"]) - PC.STRADDLE_HARD
    assert PC.STRADDLE_TIE[0] < r < sum(PC.STRADDLE_TIE)                      # the last kept pixel of the tie lies in the second tile
    lg, y, opt = PC.inputs("saturated_top", T)
    l32 = PC.pixel_losses(lg, y, opt, dtype=torch.float32)[0]
    assert set(np.unique(l32.numpy())) == {0.0, 120.0}
    for tag in ("saturated_top", "saturated_zero"):
        K, wrong = PC.kept_count(l32.numel(), PC.cases(T)[tag][5]["keep"], 0), int((l32 == 120.0).sum())
        assert (K < wrong) == (tag == "saturated_top") and 0 < K < l32.numel()
    lg, y, opt = PC.inputs("high_digit", T)
    bits = PC.pixel_losses(lg, y, opt, dtype=torch.float32)[0].numpy().view(np.uint32)
    assert (bits & 0x7FFFFF == 0).all() and len(np.unique(bits >> 23)) == 5
    lg, y, opt = PC.inputs("low_digit", T)
    l64 = PC.pixel_losses(lg, y, opt)[0]
    assert float(l64.max() - l64.min()) < 2.0 ** -13 and len(np.unique(l64.numpy())) == 128
    lg, y, opt = PC.inputs("opt_focal1_sure", T)
    p = torch.softmax(lg.double(), 1).gather(1, y.clamp_min(0)[:, None])[:, 0]
    assert int(((p == 1.0) & (y != PC.IGNORE)).sum()) > 20
    assert PC.kept_count(1, 1e-9, 0) == 1 and PC.kept_count(T + 5, 1e-9, 0) == 1          # "k1"
    assert 0.0 in PC.cases(T)["opt_weights"][5]["weight"]


@pytest.mark.parametrize("variant", PC.VARIANTS)
def test_cases_tell_wrong_readings_of_the_definition_apart(variant):
    """each wrong variant of the reference, selecting for itself, misses the value or the gradient of at least one case by more than
    the bar the kernels are held to there"""
    missed = []
    for tag in PC.cases(T):
        right = PC.reference(tag, T)
        lg, y, opt = PC.inputs(tag, T)
        l = lg.double().requires_grad_(True)
        v = PC.pixel_ce_reference(l, y, opt, variant=variant)
        v.backward()
        ev, eg = PC.err_of("value", v.detach(), right.r64["value"]), PC.err_of("grad", l.grad, right.r64["grad"])
        if ev > right.bar("value", PC.CAP["value"]) or eg > right.bar("grad", PC.CAP["grad"]):
            missed.append(tag)
    print(f"{variant}: told apart by {len(missed)} of {len(PC.cases(T))} cases, e.g. {missed[:4]}")
    assert missed, variant


def test_pinned_kept_map_reproduces_the_selection_and_ignored_pixels_get_no_gradient():
    lg, y, opt = PC.inputs("opt_all_image", T)
    l = lg.double().requires_grad_(True)
    v = PC.pixel_ce_reference(l, y, opt)
    v.backward()
    kept = PC.select(PC.pixel_losses(lg, y, opt)[0].numpy(), (y != PC.IGNORE).numpy(), opt["keep"], opt["min_kept"], opt["per_image"])
    assert float(PC.pixel_ce_reference(lg, y, opt, kept=kept)) == float(v.detach())
    g = l.grad.permute(0, 2, 3, 1)
    assert float(g[torch.as_tensor(kept != 1)].abs().max()) == 0.0 and float(g.abs().max()) > 0.0
    for b in range(2):                                                      # per image: K of each image's own counted pixels
        n = int((y[b] != PC.IGNORE).sum())
        assert int((kept[b] == 1).sum()) == PC.kept_count(n, opt["keep"], opt["min_kept"])
