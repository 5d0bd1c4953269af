"""CPU tier of the pinned training-step tests (tests/train_net_oracle.py): with torch fp32 standing in for the HIP path, on the ragged
size of a depth-2 and a depth-3 case,
  - the stand-in passes every bar tests/test_gpu_train_net.py sets (forward record, decisions, gradients, bias bound, launches derivable);
  - each mutant -- a wrong backward schedule expressed in the reference -- misses a bar by at least 10x on at least one tensor;
  - pins_from on the stand-in's record reproduces its decisions exactly."""
import pytest
import torch

import mgunet_oracle as O
import train_net_oracle as T

HOST_CASES = ["f24d2", "f32d3c1"]


@pytest.fixture(scope="module", params=HOST_CASES)
def standin(request):
    """The stand-in path (the free torch fp32 network) on the case's ragged size, and the reference for its pins, computed once."""
    case = request.param
    cfg, _ = T.CASES[case]
    shape = T.sizes(case)["ragged"]
    p = O.make_unet_params(*cfg, seed=21)
    x = torch.from_numpy(O.formula_normal(f"trainnet/{case}/x", shape, seed=21))
    _, dl = T.formula_dlogits(f"trainnet/{case}", shape, cfg[1])
    g, _, run = T.gradients(p, x, dl, cfg[3], None, torch.float32)
    pins = T.pins_from(run.record, cfg[3])
    ref, dz, bar, emu = T.reference(p, x, dl, cfg[3], pins)
    return dict(case=case, cfg=cfg, shape=shape, p=p, x=x, dl=dl, g=g, run=run, pins=pins, ref=ref, dz=dz, bar=bar, emu=emu)


def test_pins_from_reproduces_the_stand_ins_decisions(standin):
    made = T.pins_of(standin["run"])
    assert sorted(made) == sorted(standin["pins"]) and len(made) == 4 * standin["cfg"][3] + 2 + standin["cfg"][3]
    for k, v in made.items():
        assert torch.equal(v, standin["pins"][k]), k


def test_stand_in_passes_every_bar(standin):
    s = standin
    depth = s["cfg"][3]
    p64 = T.f64_params(s["p"])
    rec = T.record_ratios(p64, s["run"].record, depth)
    worst = max(rec, key=rec.get)
    print(f"    [{s['case']}] forward record: worst error / bar {rec[worst]:.3f} on {worst}")
    assert all(v <= 1.0 for v in rec.values()), {k: v for k, v in rec.items() if not v <= 1.0}
    total, differing, outside = T.compare_decisions(s["pins"], T.free_decisions(p64, s["x"], depth))
    print(f"    [{s['case']}] decisions {total}, differing from float64's {differing} ({differing / total:.1e}), outside the margins {outside}")
    assert not outside and differing / total <= T.DIFFER_CAP
    for n, e in s["emu"].items():
        k = max(e, key=e.get)
        print(f"    [{s['case']}] emulation {n}: worst error {e[k]:.2e} on {k}")
    ratio = T.judge(s["g"], s["ref"], s["dz"], s["bar"], s["case"])
    assert all(bool(torch.isfinite(v).all()) for v in s["g"].values())
    assert not T.misses(ratio), {k: ratio[k] for k in T.misses(ratio)}
    assert set(ratio) == {k for k in s["ref"]}                      # every parameter tensor is judged
    assert sum(T.backward_launches(s["cfg"], s["shape"]).values()) == 2 * (4 * depth + 2) - 1 + depth


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_mutant_misses_a_bar_tenfold(standin, mutant):
    s = standin
    g, _, _ = T.gradients(s["p"], s["x"], s["dl"], s["cfg"][3], s["pins"], torch.float64, mutant=mutant)
    ratio = T.judge(g, s["ref"], s["dz"], s["bar"], f"{s['case']} {mutant}", show=lambda *_: None)
    k = max(ratio, key=ratio.get)
    print(f"    [{s['case']}] mutant {mutant}: misses the bar {ratio[k]:.3g}-fold on {k}; {sum(r > 1 for r in ratio.values())} of {len(ratio)} tensors miss")
    assert ratio[k] >= 10.0, (mutant, k, ratio[k])


def test_launch_restatement_reaches_every_kernel_family():
    """Over the GPU matrix the host restatement of the picks names every weight-gradient and data-gradient family at least once (the GPU
    tests prove per case that the launches ARE the restatement's)."""
    seen = set()
    for case, (cfg, sw) in T.CASES.items():
        for shape in T.sizes(case).values():
            seen |= set(T.backward_launches(cfg, shape, sw))
    want = {T.WGRAD_THIN, T.WGRAD_WINO_X3, T.WGRAD_WINO, T.WGRAD_DIRECT, T.DGRAD_TILES, T.CONVT_DGRAD_X3, T.CONVT_DGRAD_TILES}
    assert want <= seen, want - seen
    assert seen & set(T.DGRAD_WINO[:2])
