"""tests/tta_oracle.py checked on the CPU: merge64 on logits that really are views of one tensor, against a gather through the host
index table, and, for every case tests/test_gpu_tta_kernels.py runs on the device, that the reference is a distribution, that the
fp32 emulation of the kernel's order stays inside bound(C, K), and that the label comparison leaves out at most 0.1 % of the pixels."""
import numpy as np
import pytest
import torch

import tta_oracle as TO
from mgunet import tta

SHAPES = [(6, 10), (10, 6), (7, 7), (1, 5), (1, 1)]


def views_of(lg, rows, B, H, W):
    """per-group logits (slots * B, Hg, Wg, C) holding the views of lg (B, H, W, C) the rows name"""
    C = lg.shape[-1]
    groups = [None if s is None else torch.zeros(s + (C,), dtype=lg.dtype) for s in TO.group_shapes(rows, B, H, W)]
    for g, slot, flip, turns in rows:
        groups[g][slot * B:(slot + 1) * B] = TO.view(lg.permute(0, 3, 1, 2), flip, turns).permute(0, 2, 3, 1)
    return groups


@pytest.mark.parametrize("name", TO.NAMED)
@pytest.mark.parametrize("H,W", SHAPES)
def test_merge_of_true_views_is_the_softmax(name, H, W):
    B, C = 2, 3
    lg = 3.0 * torch.randn((B, H, W, C), generator=torch.Generator().manual_seed(H * 100 + W))
    rows = TO.table(name, H, W)
    got = TO.merge64(views_of(lg, rows, B, H, W), rows, B, C, H, W)
    assert got.dtype == torch.float64 and got.shape == (B, H, W, C)
    assert torch.allclose(got, TO.softmax64(lg), rtol=0, atol=1e-15)


@pytest.mark.parametrize("name,H,W", [("group1_only", 6, 10), ("group1_only", 5, 1), ("mixed_slots", 6, 10), ("mixed_slots", 7, 7),
                                      ("repeat", 6, 10), ("repeat", 7, 7)])
def test_extra_tables_are_valid_and_invert(name, H, W):
    rows = TO.table(name, H, W)
    assert len(rows) in (2, 4)
    for g, slot, flip, turns in rows:
        assert g == ((turns & 1) if H != W else 0) and 0 <= slot < 8 and 0 <= flip < 4 and 0 <= turns < 4
    assert len({(g, slot) for g, slot, _, _ in rows}) == len(rows)            # no two views share a buffer
    if name == "mixed_slots":
        assert [(f, r) for _, _, f, r in rows] == [(2, 0), (1, 1), (3, 2), (0, 3)]
        assert [(g, s) for g, s, _, _ in rows] == ([(0, 3), (0, 2), (0, 1), (0, 0)] if H == W else [(0, 1), (1, 1), (0, 0), (1, 0)])
    if name == "repeat":
        assert rows[0][2:] == rows[1][2:] and rows[0][1] != rows[1][1]
    if name == "group1_only":
        assert all(g == 1 for g, _, _, _ in rows)
    lg = torch.randn((2, H, W, 4), generator=torch.Generator().manual_seed(5))
    got = TO.merge64(views_of(lg, rows, 2, H, W), rows, 2, 4, H, W)
    assert torch.allclose(got, TO.softmax64(lg), rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", TO.NAMED)
@pytest.mark.parametrize("H,W", SHAPES)
def test_merge_equals_the_host_tables_gather(name, H, W):
    """independent logits per view: merge64's unview against mgunet.tta.view_inverse_index, which test_tta_host.py ties to torch"""
    B, C = 2, 3
    rows = TO.table(name, H, W)
    groups = TO.logits("random", TO.group_shapes(rows, B, H, W), C, seed=H * 10 + W)
    want = torch.zeros((B, H, W, C), dtype=torch.float64)
    for g, slot, flip, turns in rows:
        p = TO.softmax64(groups[g][slot * B:(slot + 1) * B])                  # (B, Hg, Wg, C)
        idx = tta.view_inverse_index(flip, turns, H, W).flatten()
        want += p.flatten(1, 2)[:, idx].view(B, H, W, C)
    want /= len(rows)
    assert torch.equal(TO.merge64(groups, rows, B, C, H, W), want)


def test_case_generators():
    shapes = [(2, 3, 5), None]
    for case in TO.CASES:
        a, b = TO.logits(case, shapes, 5, 11), TO.logits(case, shapes, 5, 11)
        assert a[1] is None and a[0].dtype == torch.float32 and a[0].shape == (2, 3, 5, 5) and torch.equal(a[0], b[0]), case
    sp = TO.logits("spread", shapes, 5, 1)[0].double()
    assert float((sp[..., 0::2].amin(-1) - sp[..., 1::2].amax(-1)).min()) > 103
    dd = TO.logits("dead", shapes, 5, 1)[0]
    assert TO.dead_classes(5) == [1, 4] and bool((dd[..., [1, 4]] == -1e30).all()) and float(dd[..., [0, 2, 3]].abs().max()) < 20
    assert TO.dead_classes(1) == [] and TO.dead_classes(2) == [1]
    assert bool((TO.logits("equal", shapes, 5, 1)[0] == 7.25).all())
    tt = TO.logits("tie_top", shapes, 5, 1)[0]
    rest = tt[..., [0, 2, 3]].amax(-1)
    assert torch.equal(tt[..., 1], tt[..., 4]) and bool((tt[..., 1] >= rest + 1.0).all())
    oh = TO.logits("one_hot", shapes, 5, 1)[0]
    assert bool(((oh == 0).sum(-1) == 1).all()) and set(oh.unique().tolist()) == {0.0, -200.0}
    assert float(TO.logits("huge", shapes, 5, 1)[0].min()) > 2.9e4


@pytest.mark.parametrize("C", TO.MERGE_CLASSES)
@pytest.mark.parametrize("case", TO.FLOAT_CASES)
def test_device_cases_reference_emulation_and_margins(case, C):
    worst, share_max = 0.0, 0.0
    for name, (H, W), B in TO.LAYOUTS:
        rows, groups = TO.make(case, C, name, H, W, B)
        K = len(rows)
        ref = TO.merge64(groups, rows, B, C, H, W)
        assert float((ref.sum(-1) - 1.0).abs().max()) <= 1e-12
        for c in (TO.dead_classes(C) if case == "dead" else []):
            assert bool((ref[..., c] == 0.0).all())
        emu = torch.from_numpy(TO.emulate32(groups, rows, B, C, H, W))
        d = float((emu.double() - ref).abs().max())
        worst = max(worst, d / TO.bound(C, K))
        assert d <= TO.bound(C, K), (name, H, W, B, d, TO.bound(C, K))
        share = float((TO.margin(ref) <= 2 * TO.bound(C, K)).double().mean())
        share_max = max(share_max, share)
        if case != "spread":                       # spread is compared on probabilities only where classes nearly tie
            assert share <= 1e-3, (name, H, W, B, share)
        keep = TO.margin(ref) > 2 * TO.bound(C, K)
        assert torch.equal(emu.argmax(-1)[keep], ref.argmax(-1)[keep])
    print(f"[tta emulation C={C} {case}] max|emulation - merge64| / bound = {worst:.3f}, "
          f"largest share of pixels left out of the label check = {100 * share_max:.3f} %")


@pytest.mark.parametrize("C", TO.EXACT_CLASSES)
def test_one_hot_cases_are_exact(C):
    for name, (H, W), B in TO.EXACT_LAYOUTS:
        rows, groups = TO.make("one_hot", C, name, H, W, B)
        K = len(rows)
        ref = TO.merge64(groups, rows, B, C, H, W)
        ref32 = ref.float()                                   # exp(-200) = 1.4e-87 in the float64 reference rounds away here
        assert torch.equal(ref32 * K, torch.round(ref32 * K)) and bool((ref32.sum(-1) == 1.0).all())
        assert float((ref.sum(-1) - 1.0).abs().max()) <= 1e-12
        emu = TO.emulate32(groups, rows, B, C, H, W)
        assert np.array_equal(emu, ref32.numpy())


@pytest.mark.parametrize("C", TO.MERGE_CLASSES)
def test_tie_cases_in_the_emulation(C):
    for name, (H, W), B in TO.LAYOUTS:
        if C >= 3:
            rows, groups = TO.make("tie_top", C, name, H, W, B)
            emu = torch.from_numpy(TO.emulate32(groups, rows, B, C, H, W))
            a, b = TO.tie_classes(C)
            assert torch.equal(emu[..., a], emu[..., b]) and bool((emu.argmax(-1) == a).all())
        rows, groups = TO.make("equal", C, name, H, W, B)
        emu = TO.emulate32(groups, rows, B, C, H, W)
        assert bool((emu == np.float32(1) / np.float32(C)).all())
