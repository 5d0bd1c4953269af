"""tests/optim_cases.py without a GPU: the cases are what they claim to be and the bars can fail -- the arithmetic of csrc/optim.hip
restated in numpy meets them on every case, and each of five wrong variants (L2 decay in place of decoupled, the clip factor from
the unscaled gradient's norm, the clip applied after the decay term, bias corrections from the attempted-step count, a sum of
squares kept in fp32) misses them on at least one.  Then what needs no kernel at all: the schedulers against torch's own, the
config mapping with the Trainer's construction stubbed, the AdamW state layout, the header's new entry points."""
import math

import numpy as np
import pytest
import torch

import mgunet
import optim_cases as OC
from mgunet import engine

ids = lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c)


# ---- the gradient norm --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", OC.NORM_RUNS, ids=ids)
def test_norm_inputs_are_what_they_claim(run):
    content, n = run
    g = OC.norm_input(content, n)
    ref = OC.norm_reference(content, n)
    assert g.dtype == torch.float32 and tuple(g.shape) == (n,)
    sq32 = (g * g)
    if content == "one_1e19":
        # 1e38: a factor 3.4 below the largest fp32 value (four such elements overflow an fp32 sum), 44 orders above the rest
        assert float(sq32.max()) > 2.0 ** 126 and math.isfinite(ref) and ref > 1e37
    if content == "all_1e-30":
        assert not bool(sq32.any()) and ref > 0.0                                        # every square underflows fp32
    if content == "zero":
        assert ref == 0.0
    # a plain numpy sum in double is within the bar; a sum kept in fp32 is not, wherever fp32 cannot hold the squares
    assert OC.sumsq_err(float(np.sum(g.double().numpy() ** 2)), ref) <= OC.sumsq_bar(n)
    if content in ("one_1e19", "all_1e-30"):
        with np.errstate(over="ignore"):
            assert OC.sumsq_err(float(np.sum(g.numpy() * g.numpy(), dtype=np.float32)), ref) > OC.sumsq_bar(n)


def test_norm_sizes_pass_the_grid_and_a_chunk_boundary():
    assert max(OC.OPT_SIZES) == OC.OPT_GRID + 1 and 1 in OC.OPT_SIZES
    assert {n for _, n in OC.NORM_RUNS} == set(OC.OPT_SIZES) and {c for c, _ in OC.NORM_RUNS} == set(OC.NORM_CONTENTS)


# ---- the chains ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", OC.RUNS, ids=ids)
def test_chain_case_conditions_and_the_kernel_arithmetic(run):
    tag, n = run
    kind, mom, wd, gs, clip, ema, warm, mag, bad = OC.CASES[tag]
    ref, cap = OC.reference(tag, n), OC.opt_cap()
    p, grads, max_norm = OC.inputs(tag, n)
    assert len([g for g in grads if OC.finite(g)]) == OC.OPT_STEPS and len(grads) == OC.OPT_STEPS + (bad is not None)
    assert float(np.float32(max_norm)) == max_norm and float(np.abs(ref.r64["p"]).max()) > 1e-7
    assert float(p.abs().max()) <= 2.0 ** -7                                             # rounding p cannot reach the bar
    coefs = OC.clip_coefs(tag, n)
    if clip in ("half", "one"):
        assert all(c < 1.0 for c in coefs), coefs
    if clip == "far":
        assert all(c == 1.0 for c in coefs) and max_norm > 0
    if clip == "edge":
        norm0 = OC.scaled_norm64(grads[0], gs)
        assert abs(max_norm - norm0) <= 1e-3 * norm0 and max_norm > 0
    if clip == "off":
        assert max_norm == 0.0
    if kind == "adamw":
        assert wd == 1e-2
    assert set(ref.r64) == {"p"} | ({"m", "v"} if kind != "sgd" else ({"buf"} if mom else set())) | ({"ema"} if ema else set())
    got = OC.formula32(tag, n)
    for k in ref.r64:
        err, bar = OC.err_of(k, got[k], ref.r64[k]), ref.bar(k, cap)
        print(f"| optim {tag} n={n} | {k} | {ref.cond[k]:.1e} | {bar:.1e} | {err:.1e} |")
        assert bar <= cap and err <= bar, (k, err, bar)


def test_chain_cases_cover_the_sweep():
    for tag in OC.SWEPT:
        assert {n for t, n in OC.RUNS if t == tag} == set(OC.OPT_SIZES)
    assert {t for t, _ in OC.RUNS} == set(OC.CASES)
    kinds = {(c[0], c[1] != 0.0, c[4] != "off") for c in OC.CASES.values()}
    for kind, mom in (("adam", False), ("adamw", False), ("sgd", False), ("sgd", True)):
        assert (kind, mom, False) in kinds and (kind, mom, True) in kinds
    clips = {c[4] for c in OC.CASES.values()}
    assert {"half", "far", "edge"} <= clips
    assert any(c[3] == 0.125 and c[4] == "half" for c in OC.CASES.values()) and any(c[8] is not None for c in OC.CASES.values())
    assert any(c[6] for c in OC.CASES.values())                                          # an EMA warm-up


@pytest.mark.parametrize("variant,tag", [("l2_for_decoupled", "adamw"), ("l2_for_decoupled", "adamw_clip"),
                                         ("clip_unscaled_norm", "adam_gs8_clip"), ("clip_after_decay", "adam_clip"),
                                         ("clip_after_decay", "sgd_m0_clip"), ("attempted_step_count", "adam_skip"),
                                         ("sumsq_fp32", "sgd_huge_clip")])
def test_wrong_variants_fall_outside_the_bar(variant, tag):
    n = 100003
    assert not OC.outside_bar(tag, n, "kernel")
    assert OC.outside_bar(tag, n, variant), (variant, tag)


def test_every_wrong_variant_is_tried():
    tried = {"l2_for_decoupled", "clip_unscaled_norm", "clip_after_decay", "attempted_step_count", "sumsq_fp32"}
    assert tried | {"kernel"} == set(OC.VARIANTS)


def test_decoupled_and_l2_decay_differ_by_more_than_the_bar():
    for tag in ("adamw", "adamw_clip", "adamw_far", "adamw_edge"):
        ref, cap = OC.reference(tag, 100003), OC.opt_cap()
        l2 = OC.formula32(tag, 100003, "l2_for_decoupled")
        assert OC.err_of("m", l2["m"], ref.r64["m"]) > ref.bar("m", cap), tag


# ---- schedulers ---------------------------------------------------------------------------------------------------------------------
def _torch_optimizer(lr):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)


@pytest.mark.parametrize("T_max,eta_min,lr", [(7, 0.0, 1e-3), (10, 1e-5, 0.05), (1, 0.0, 1e-3)])
def test_cosine_annealing_equals_torch(T_max, eta_min, lr):
    opt = _torch_optimizer(lr)
    want = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max, eta_min=eta_min)
    holder = OC.LrHolder(lr)
    mine = mgunet.CosineAnnealingLR(holder, T_max, eta_min)
    assert mine.get_last_lr() == want.get_last_lr()
    for epoch in range(2 * T_max + 3):
        opt.step()
        want.step()
        mine.step()
        assert mine.get_last_lr() == want.get_last_lr(), epoch
    other = mgunet.CosineAnnealingLR(OC.LrHolder(lr), T_max, eta_min)                    # the state round trip continues the sequence
    other.load_state_dict(mine.state_dict())
    for _ in range(3):
        opt.step()
        want.step()
        other.step()
        assert other.get_last_lr() == want.get_last_lr()


@pytest.mark.parametrize("script", OC.PLATEAU_SCRIPTS, ids=lambda s: f"{s[0]}-{s[1]}")
def test_reduce_on_plateau_equals_torch(script):
    mode, tmode, metrics = script
    lr = 1e-3
    opt = _torch_optimizer(lr)
    want = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode=mode, threshold_mode=tmode, **OC.PLATEAU_KW)
    holder = OC.LrHolder(lr)
    mine = mgunet.ReduceLROnPlateau(holder, mode=mode, threshold_mode=tmode, **OC.PLATEAU_KW)
    seen = []
    for i, v in enumerate(metrics):
        want.step(v)
        mine.step(v)
        assert mine.get_last_lr() == [opt.param_groups[0]["lr"]], (i, v)
        assert (mine.best, mine.num_bad_epochs, mine.cooldown_counter) == (want.best, want.num_bad_epochs, want.cooldown_counter), i
        seen.append(holder.lr)
        if i == len(metrics) // 2:
            clone = mgunet.ReduceLROnPlateau(OC.LrHolder(0.0), mode=mode, threshold_mode=tmode)
            clone.load_state_dict(mine.state_dict())
            assert clone.state_dict() == mine.state_dict()
    if (mode, tmode) == ("min", "rel"):                                                  # the script that reaches the floor
        assert len(set(seen)) >= 4 and min(seen) > OC.PLATEAU_KW["min_lr"]               # the last cut, below eps, is not made
        assert min(seen) * OC.PLATEAU_KW["factor"] < OC.PLATEAU_KW["min_lr"]
    else:
        assert len(set(seen)) >= 2


def test_scheduler_argument_errors():
    with pytest.raises(ValueError):
        mgunet.ReduceLROnPlateau(OC.LrHolder(1.0), factor=1.0)
    with pytest.raises(ValueError):
        mgunet.ReduceLROnPlateau(OC.LrHolder(1.0), mode="best")
    with pytest.raises(ValueError):
        mgunet.ReduceLROnPlateau(OC.LrHolder(1.0), threshold_mode="both")


# ---- the config mapping, Trainer's construction stubbed -----------------------------------------------------------------------------
class _Recorder:
    def __init__(self, model, **kw):
        self.model, self.kw, self.lr = model, kw, kw.get("lr", 1e-3)

    def set_lr(self, lr):
        self.lr = lr


@pytest.fixture
def stub_trainer(monkeypatch):
    monkeypatch.setattr(engine, "Trainer", _Recorder)


def test_trainer_from_config_accepts_the_reference_spellings(stub_trainer):
    model = object()
    for name, want in (("AdamW", "adamw"), ("adam", "adam"), ("SGD", "sgd"), ("Adam", "adam"), ("adamw", "adamw")):
        t = mgunet.trainer_from_config(model, {"optimizer": name})
        assert t.model is model and t.kw == {"optimizer": want}
    with pytest.raises(ValueError):
        mgunet.trainer_from_config(model, {"optimizer": "rmsprop"})
    assert mgunet.trainer_from_config(model, {}).kw == {"optimizer": "adam"}


def test_trainer_from_config_maps_every_key(stub_trainer):
    cfg = {"optimizer": "AdamW", "learning_rate": 3e-4, "weight_decay": 1e-2, "sgd_momentum": 0.8, "grad_clip_norm": 0.5, "ema_decay": 0.999,
           "accumulate_steps": 4, "skip_nonfinite": True, "batch_size": 16, "lr_scheduler": "StepLR"}
    t = mgunet.trainer_from_config(object(), cfg)
    assert t.kw == {"optimizer": "adamw", "lr": 3e-4, "weight_decay": 1e-2, "momentum": 0.8, "max_grad_norm": 0.5, "ema_decay": 0.999,
                    "accumulate": 4, "skip_nonfinite": True}
    t = mgunet.trainer_from_config(object(), cfg, lr=1.0, loss="ce+dice")                 # overrides win
    assert t.kw["lr"] == 1.0 and t.kw["loss"] == "ce+dice" and t.kw["accumulate"] == 4
    shipped = mgunet.load_config(engine._lib.PKG_ROOT + "/configs", "training.yaml")
    t = mgunet.trainer_from_config(object(), shipped)                                     # absent keys stay off
    assert t.kw == {"optimizer": "adam", "lr": 0.001, "weight_decay": 0.0001, "momentum": 0.9}


def test_scheduler_from_config_maps_every_key():
    tr = OC.LrHolder(1e-3)
    s = mgunet.scheduler_from_config(tr, {"lr_scheduler": "StepLR", "lr_step_size": 7, "lr_gamma": 0.3})
    assert isinstance(s, mgunet.StepLR) and (s.step_size, s.gamma) == (7, 0.3)
    s = mgunet.scheduler_from_config(tr, {"lr_scheduler": "CosineAnnealingLR", "lr_t_max": 12, "lr_eta_min": 1e-6})
    assert isinstance(s, mgunet.CosineAnnealingLR) and (s.T_max, s.eta_min) == (12, 1e-6)
    s = mgunet.scheduler_from_config(tr, {"lr_scheduler": "CosineAnnealingLR", "num_epochs": 100})
    assert (s.T_max, s.eta_min) == (100, 0.0)
    s = mgunet.scheduler_from_config(tr, {"lr_scheduler": "ReduceLROnPlateau", "lr_patience": 3, "lr_factor": 0.25})
    assert isinstance(s, mgunet.ReduceLROnPlateau) and (s.patience, s.factor) == (3, 0.25)
    assert mgunet.scheduler_from_config(tr, {}) is None
    with pytest.raises(ValueError):
        mgunet.scheduler_from_config(tr, {"lr_scheduler": "OneCycleLR"})
    with pytest.raises(ValueError):
        mgunet.scheduler_from_config(tr, {"lr_scheduler": "CosineAnnealingLR"})
    shipped = mgunet.load_config(engine._lib.PKG_ROOT + "/configs", "training.yaml")
    s = mgunet.scheduler_from_config(tr, shipped)
    assert isinstance(s, mgunet.StepLR) and (s.step_size, s.gamma) == (30, 0.1)


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def test_adamw_state_layout_loads_into_torch():
    ps = [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5))]
    m, v = torch.arange(11.0), torch.arange(11.0) * 2
    sd = mgunet.adam_state_dict(ps, m, v, 4, 1e-3, (0.9, 0.999), 1e-8, 1e-2, decoupled=True)
    opt = torch.optim.AdamW(ps, lr=0.5)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g["lr"] == 1e-3 and g["weight_decay"] == 1e-2 and g.get("decoupled_weight_decay", True) is True
    assert torch.equal(opt.state[ps[1]]["exp_avg"], m[6:]) and float(opt.state[ps[0]]["step"]) == 4.0
    assert set(sd["param_groups"][0]) == set(torch.optim.AdamW(ps).state_dict()["param_groups"][0])
    assert mgunet.adam_state_dict(ps, m, v, 4, 1e-3, (0.9, 0.999), 1e-8, 1e-2)["param_groups"][0]["decoupled_weight_decay"] is False


def test_header_declares_the_entry_points_and_the_descriptor_matches():
    import ctypes as C
    protos = mgunet._lib.parse_header()
    assert protos["mgu_optim_step"] == (C.c_int, [C.c_void_p] * 8 + [C.c_int64, C.c_void_p], True)
    assert protos["mgu_grad_norm"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p], True)
    assert protos["mgu_grad_accumulate"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p], True)
    assert protos["mgu_grad_norm_chunk"] == (C.c_int64, [C.c_int64], False) and protos["mgu_grad_norm_blocks"] == (C.c_int, [C.c_int64], False)
    D = mgunet._lib.OptimDesc
    assert [f[0] for f in D._fields_] == ["kind", "lr", "beta1", "beta2", "eps", "weight_decay", "momentum", "grad_scale", "max_norm",
                                          "skip_nonfinite", "ema_decay", "ema_warmup"]
    assert (D.beta1.offset, D.eps.offset, D.ema_warmup.offset, C.sizeof(D)) == (8, 24, 52, 56)
    hdr = open(mgunet._lib.HEADER).read()
    assert "#define MGU_OPTIM_CTRL_BYTES 64" in hdr and mgunet._lib.OPTIM_CTRL_BYTES == 64
    for name, code in mgunet._lib.OPTIM_KINDS.items():
        assert f"#define MGU_OPTIM_{name.upper()} {code}" in hdr


def test_option_checks_need_no_device():
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            engine._DeviceStep._check_step_options(bad, 0.0)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            engine._DeviceStep._check_step_options(0.0, bad)
    engine._DeviceStep._check_step_options(0.0, 0.0)
    engine._DeviceStep._check_step_options(2.5, 0.999)
