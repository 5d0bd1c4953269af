"""CPU checks of tests/fp32_oracle.py, the yardstick of tests/test_gpu_fp32_layers.py: the derived kernel forms against hand-written
expectations, the two correct fp32 emulations under bar (a) and on the exact data, and every emulated indexing fault caught by both."""
import pytest
import torch

import fp32_oracle as P
import mgunet_oracle as O

ORDER = ["f16d2", "f24d1c4", "f24d2", "f32d1c4", "f32d3c1", "f48d1c1", "f64d1", "f80d1", "f96d1"]        # cheapest first (f96d1_direct: same arithmetic)


def one_image(shape):
    return (1,) + tuple(shape[1:])


def test_layer_forms_of_two_cases_by_hand():
    asm = "wino_asm_"
    want = {
        ("f24d2", "whole"): [("tiles", 3, 24), ("tiles", 24, 24), ("maxpool2", 24, 24), ("tiles", 24, 48), ("wino_cp2+pool", 48, 48),
                             ("wino_cp2", 48, 96), ("wino_cp2", 96, 96), ("convt_generic", 96, 48), ("wino_cp2", 96, 48), ("wino_cp2", 48, 48),
                             ("convt_generic", 48, 24), ("wino_cp1", 48, 24), ("tiles", 24, 24), ("head", 24, 2), ("patch_mean", 24, 24)],
        ("f32d1c4", "whole"): [("first_valu", 4, 32), (asm + "cp1r2+pool", 32, 32), ("wino_cp2", 32, 64), ("wino_cp2", 64, 64),
                               ("convt_x3", 64, 32), (asm + "cp1r4", 64, 32), (asm + "cp1r2_head", 32, 32), ("patch_sum_combine", 32, 32)],
        ("f32d1c4", "ragged"): [("first_valu", 4, 32), ("wino_cp1+pool", 32, 32), ("wino_cp2", 32, 64), ("wino_cp2", 64, 64),
                                ("convt_x3", 64, 32), ("wino_cp1", 64, 32), ("wino_cp1", 32, 32), ("patch_mean_head", 32, 4)],
    }
    want[("f24d2", "ragged")] = want[("f24d2", "whole")]            # no width of this case is eligible for assembly at any size
    for (case, size), forms in want.items():
        cfg = P.CASES[case][0]
        assert P.layer_forms(cfg, P.sizes(case)[size], P.SWITCHES.get(case)) == forms, (case, size)
    assert P.family_launches(P.CASES["f32d1c4"][0], P.sizes("f32d1c4")["whole"]) == {
        "conv3x3_first_kernel": 1, P.RECORD["wino_asm_cp1r2"]: 1, "wino3x3_cp_kernel<2>": 2, "convt2x2_x3_kernel": 1, P.RECORD["wino_asm_cp1r4"]: 1,
        P.RECORD["wino_asm_cp1r2_head"]: 1, "patch_sum_combine_kernel": 1}
    direct = P.layer_forms(P.CASES["f96d1_direct"][0], P.sizes("f96d1_direct")["ragged"], P.SWITCHES["f96d1_direct"])
    assert direct == [("tiles", 3, 96), ("halo+pool", 96, 96), ("halo", 96, 192), ("halo", 192, 192), ("convt_x3", 192, 96), ("halo", 192, 96),
                      ("halo", 96, 96), ("head", 96, 3), ("patch_mean", 96, 96)]


@pytest.mark.parametrize("case", list(P.CASES))
def test_every_listed_form_is_reached_at_some_size(case):
    cfg, listed = P.CASES[case]
    reached = {f for shape in P.sizes(case).values() for f in P.layer_forms(cfg, shape, P.SWITCHES.get(case))}
    assert not [f for f in listed if f not in reached], (case, [f for f in listed if f not in reached])


@pytest.mark.parametrize("case", ORDER)
def test_correct_emulations_pass_the_bar_and_are_exact_on_exact_data(case):
    cfg = P.CASES[case][0]
    depth = cfg[3]
    for size in ("small", "ragged"):
        if size not in P.sizes(case):
            continue
        shape = one_image(P.sizes(case)[size])
        p64 = P.f64_params(O.make_unet_params(*cfg, seed=21))
        x = torch.from_numpy(O.formula_normal(f"fp32layers/{case}/x", shape, seed=21))
        for name, emu in P.EMULATIONS.items():
            fig = P.judge(p64, depth, x, P.network(p64, x, depth, emu), f"{case} {size} {name}")
            assert not P.misses(fig), (case, size, name, fig)
        pe = P.exact_params(cfg, 1)
        xe = P.exact_input(shape, 1)
        ref = P.exact_reference(pe, xe, depth)
        assert max(float(t.abs().max()) for t in ref[1] + ref[2]) < 256
        for name in ("winograd_f2x2_3x3", "library_order_direct"):
            got = P.network(P.f64_params(pe), xe, depth, P.EMULATIONS[name], eps=P.EXACT_EPS)
            assert not P.differing(got, ref), (case, size, name, P.differing(got, ref))


def test_the_float64_network_meets_both_with_nothing_to_spare():
    cfg = P.CASES["f16d2"][0]
    shape = one_image(P.sizes("f16d2")["ragged"])
    p64 = P.f64_params(O.make_unet_params(*cfg, seed=21))
    x = torch.from_numpy(O.formula_normal("fp32layers/f16d2/x", shape, seed=21))
    fig = P.judge(p64, cfg[3], x, P.network(p64, x, cfg[3], P.EXACT), "f16d2 ragged float64", show=lambda s: None)
    assert all(worst == 0 for _, worst, _ in fig.values())
    pe, xe = P.exact_params(cfg, 0), P.exact_input(shape, 0)
    assert not P.differing(P.network(P.f64_params(pe), xe, cfg[3], P.EXACT, eps=P.EXACT_EPS), P.exact_reference(pe, xe, cfg[3]))


@pytest.mark.parametrize("mutant", list(P.MUTANTS))
def test_every_indexing_mutant_fails_the_bar_and_breaks_equality(mutant):
    """The float64 mutant network as `got`: the first (case, size), cheapest first, on which it misses bar (a) AND differs on exact data.
    A mutant no case sees means a case is missing."""
    ops = P.MUTANTS[mutant]
    for case in ORDER:
        cfg = P.CASES[case][0]
        depth = cfg[3]
        for size in ("small", "ragged"):
            if size not in P.sizes(case):
                continue
            shape = one_image(P.sizes(case)[size])
            pe, xe = P.exact_params(cfg, 1), P.exact_input(shape, 1)
            broken = P.differing(P.network(P.f64_params(pe), xe, depth, ops, eps=P.EXACT_EPS), P.exact_reference(pe, xe, depth))
            if not broken:
                continue
            p64 = P.f64_params(O.make_unet_params(*cfg, seed=21))
            x = torch.from_numpy(O.formula_normal(f"fp32layers/{case}/x", shape, seed=21))
            fig = P.judge(p64, depth, x, P.network(p64, x, depth, ops), f"{mutant} on {case} {size}", show=lambda s: None)
            if P.misses(fig):
                print(f"    {mutant}: caught on {case} {size}: bar (a) missed on {P.misses(fig)} (worst "
                      f"{max(w for _, w, _ in fig.values()):.3g} x the bar), equality (b) broken on {broken}")
                return
    raise AssertionError(f"{mutant}: no case sees it under both checks")
