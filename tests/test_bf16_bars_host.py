"""Calibration of the per-element bar of tests/bf16_oracle.py and construction checks of its exact-data networks, on the CPU.

For every case of the shape matrix (bf16_oracle.CASES), against the float64 segment reference:
  * every CORRECT float32 emulation (bf16_oracle.EMULATIONS: chunk orders, tap-major / channel-major, fma / multiply-then-add) passes
    check() on every segment and size, with a factor 2 of room in the mismatch share and K_FLOOR at least the worst coincidence
    observed plus one;
  * every MUTANT fails on every case on which it changes the arithmetic at all; none is inapplicable everywhere;
  * the limits are no looser than the older bar (>= 90 % equal, <= 1 % of max).
The exact-data networks: float64 (BatchNorm scale exactly 1), float32 and the storage emulation are bit-equal, every stored value is
an integer of at most 255, no exposed tensor has died, the nonzero positions cover every (tap, cin) over the seeds, and every
indexing mutant changes some exposed tensor of some seed."""
import functools

import pytest
import torch

import bf16_oracle as B
import mgunet_oracle as O

RAGGED = {"f32d2": (3, 37, 45)}      # (batch, H, W); every other case: 2 x 50 x 70


def sizes(case):
    cin = B.CASES[case][0][0]
    b, h, w = RAGGED.get(case, (2, 50, 70))
    if B.CASES[case][0][3] > 2:     # four halvings: no size below a patch leaves a bottleneck; 50 x 70 has 12 x 17, 6 x 8 and 3 x 4 below it
        return {"ragged": (b, cin, h, w), "whole": (1, cin, 64, 96)}
    return {"small": (2, cin, 12, 20), "ragged": (b, cin, h, w), "whole": (1, cin, 64, 96)}


@functools.lru_cache(maxsize=None)
def formula_chain(case, size):
    cfg = B.CASES[case][0]
    p = O.make_unet_params(*cfg, seed=21)
    x = torch.from_numpy(O.formula_normal(f"bf16layers/{case}/x", sizes(case)[size], seed=21))
    first = B.first_fp32_weights(cfg[0], cfg[2])
    return cfg, p, first, B.chain(p, cfg[3], x, first)


@functools.lru_cache(maxsize=None)
def run_mutant(case, mname):
    return run(case, "ragged", B.MUTANTS[mname])


def run(case, size, ops):
    cfg, p, first, ch = formula_chain(case, size)
    out = {}
    for name, (ref, fl, src) in ch.items():
        got = B.segment(p, cfg[3], name, src, first, ops)[0]
        out[name] = (B.measure(got, ref, fl, B.is_deep(cfg[3], name)), not torch.equal(got, ref))
    return out


def test_layer_forms_contain_what_each_case_claims():
    for case, (cfg, claims) in B.CASES.items():
        forms = B.layer_forms(cfg)
        for c in claims:
            assert c in forms, (case, c, forms)
    assert B.family_launches((3, 2, 32, 4)) == {"conv3x3_first_mfma_kernel": 1, "conv3x3_halo_kernel<bf16>": 17, "convt2x2_bf16_kernel": 4}


def test_limits_are_no_looser_than_the_older_bar():
    assert B.LIMITS["shallow"]["mismatch"] <= 0.10 and B.MAX_REL_LIMIT <= 1e-2
    # (deep segments: see the note at bf16_oracle.LIMITS -- no plain share holds them; the older test keeps its >= 90 % on its shapes)


def calibrate_correct(case, size_names):
    """Worst figures of the correct emulations per segment class; every one must pass."""
    keys = ("mismatch", "beyond_ulp", "beyond_floor", "k_needed")
    worst = {"shallow": dict.fromkeys(keys, 0.0), "deep": dict.fromkeys(keys, 0.0)}
    for size in size_names:
        for ename, ops in B.EMULATIONS.items():
            for name, (fig, _) in run(case, size, ops).items():
                assert B.passes(fig), (case, size, ename, name, B.failures(fig), fig)
                w = worst["deep" if fig["deep"] else "shallow"]
                for key in w:
                    w[key] = max(w[key], fig[key])
    for cls, w in worst.items():
        lim = B.LIMITS[cls]
        share = "mismatch" if cls == "shallow" else "beyond_floor"      # the calibrated share of the class
        print(f"[{case}] worst correct emulation, {cls} segments: mismatch {w['mismatch']*100:.4f} %, beyond one ulp {w['beyond_ulp']*100:.4f} %, "
              f"beyond one ulp and one floor {w['beyond_floor']*100:.4f} %; limit on {share}: {lim[share]*100:.2f} %; coincidence k "
              f"{w['k_needed']:.2f} (k {lim['k']:g})")
        assert w["k_needed"] + 1.0 <= lim["k"], "k at least the worst coincidence observed plus one"
        assert 2.0 * w[share] <= lim[share], "a factor 2 of room in the calibrated share"
    return worst


@pytest.mark.parametrize("case", list(B.CASES))
def test_bar_passes_correct_emulations_and_fails_mutants(case):
    calibrate_correct(case, ("ragged",) if case == "f32d1" else tuple(sizes(case)))
    best = None
    for mname, ops in B.MUTANTS.items():
        res = run_mutant(case, mname)
        if not any(changed for _, changed in res.values()):
            print(f"[{case}] {mname}: not applicable (changes nothing on this case)")
            continue
        failed = {name: B.failures(fig) for name, (fig, _) in res.items() if B.failures(fig)}
        margin = max(max(fig["beyond_floor"] / B.LIMITS["deep"]["beyond_floor"] if fig["deep"] else fig["mismatch"] / B.LIMITS["shallow"]["mismatch"],
                         fig["worst"]) for fig, _ in res.values())
        mis = max(fig["mismatch"] for fig, _ in res.values())
        wst = max(fig["worst"] for fig, _ in res.values())
        print(f"[{case}] {mname}: mismatch up to {mis*100:.3f} %, worst element {wst:.2f} units -> {margin:.1f} x the bar; fails on {sorted(failed)}")
        assert failed, (case, mname, "changes the arithmetic and passes the bar")
        if best is None or margin < best[0]:
            best = (margin, mname)
    print(f"[{case}] best mutant: {best[1]} at {best[0]:.1f} x the bar")


@pytest.mark.parametrize("case", list(B.CASES))
def test_bar_passes_a_whole_run_judged_as_the_gpu_tests_judge_it(case):
    """The GPU tests take every segment's predecessors from the implementation under test.  Stand-in for it: the float32 storage
    emulation of the oracle run through the whole network (its flips ride along from segment to segment)."""
    cfg = B.CASES[case][0]
    depth, first = cfg[3], B.first_fp32_weights(cfg[0], cfg[2])
    p = O.make_unet_params(*cfg, seed=21)
    for size, shape in sizes(case).items():
        x = torch.from_numpy(O.formula_normal(f"bf16layers/{case}/x", shape, seed=21))
        with torch.no_grad():
            _, sk, ft = O.unet_forward_bf16_storage(p, x, depth, first_fp32=first)
        for name in B.segment_names(depth):
            got = (sk if name.startswith("skip") else ft)[int(name[4:])]
            ref, floor = B.segment(p, depth, name, B.sources(depth, name, x, sk, ft), first)
            B.check(got, ref, floor, f"{case} {size} {name}", deep=B.is_deep(depth, name))


OLDER = {"b": ((3, 3, 8, 2), (2, 3, 37, 45)), "c": ((3, 2, 8, 3), (2, 3, 64, 48)), "f16": ((3, 2, 16, 3), (2, 3, 96, 80))}


@pytest.mark.parametrize("tag", list(OLDER))
def test_bar_passes_correct_emulations_on_the_older_bf16_cases(tag, monkeypatch):
    """The shapes of tests/test_gpu_bf16.py::test_bf16_kernels_vs_storage_emulation that a CPU reaches (its 512^2 case has the
    widths of f32d4)."""
    cfg, shape = OLDER[tag]
    monkeypatch.setitem(B.CASES, "older_" + tag, (cfg, []))
    monkeypatch.setitem(RAGGED, "older_" + tag, shape[:1] + shape[2:])
    calibrate_correct("older_" + tag, ("ragged",))


def test_no_mutant_is_inapplicable_everywhere():
    for mname in B.MUTANTS:
        assert any(changed for case in B.CASES for _, changed in run_mutant(case, mname).values()), mname


@pytest.mark.parametrize("case", list(B.CASES))
def test_exact_data_networks(case):
    cfg = B.CASES[case][0]
    depth = cfg[3]
    shapes = [s for k, s in sizes(case).items() if not (case == "f32d1" and k != "ragged")]
    cover = {}
    changed = {m: False for m in B.INDEXING}
    for seed in range(B.exact_seeds(cfg)):
        p = B.exact_params(cfg, seed)
        for name, w in p.items():
            if name.endswith("conv1.weight") or name.endswith("conv2.weight") or name.endswith("upsample.weight"):
                nz = (w != 0).any(dim=1 if name.endswith("upsample.weight") else 0)      # over the output channels
                cover[name] = cover.get(name, torch.zeros_like(nz)) | nz
                assert not torch.equal(w, w.flip(-1)) and not torch.equal(w, w.flip(-2)) and not torch.equal(w, w.transpose(-1, -2))
        for shape in shapes:
            x = B.exact_input(shape, seed)
            lg, sk, ft = B.exact_reference(p, x, depth)
            with torch.no_grad():
                lg32, sk32, ft32 = O.unet_forward(p, x, depth, eps=1e-30)
                lge, ske, fte = O.unet_forward_bf16_storage(p, x, depth, first_fp32=True)
            for a, b, c in zip([lg] + sk + ft, [lg32] + sk32 + ft32, [lge] + ske + fte):
                assert torch.equal(a, b.double()) and torch.equal(a, c.double()), (case, seed, shape)
            for t in sk + ft:
                assert torch.equal(t, t.round()) and float(t.abs().max()) <= 255, (case, seed, shape, float(t.abs().max()))
                assert float((t != 0).double().mean()) >= 0.25 and t.unique().numel() >= 8, (case, seed, shape)
            assert torch.equal(lg, lg.round()) and float(lg.abs().max()) < 2 ** 24
            if shape != sizes(case)["ragged"]:
                continue
            ch = B.chain(p, depth, x, False)
            for (name, (ref, _, src)), want in zip(ch.items(), sk + ft[::-1]):
                assert torch.equal(ref, want), (case, seed, name, "segment() gives the one right answer on exact data")
            for m in B.INDEXING:
                if not changed[m]:
                    changed[m] = any(not torch.equal(B.segment(p, depth, name, src, False, B.MUTANTS[m])[0], ref)
                                     for name, (ref, _, src) in ch.items())
    for name, c in cover.items():
        assert bool(c.all()), (case, name, "a (tap, cin) position is zero under every seed")
    for m in B.INDEXING:
        applicable = any(ch for _, ch in run_mutant(case, m).values())
        assert changed[m] or not applicable, (case, m, "an indexing fault the exact data cannot see")
    print(f"[{case}] exact data: {B.exact_seeds(cfg)} seeds, indexing mutants seen: {[m for m in B.INDEXING if changed[m]]}")
