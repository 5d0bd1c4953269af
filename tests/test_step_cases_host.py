"""tests/step_cases.py without a GPU: the cases are what they claim to be, and the bars can fail -- the formulas the loss kernels and
launch_adam used before (restated in numpy fp32 in the cases module, for this file only) miss them on the logits and weights of a
trained network and meet them on the random inputs the older tests use, while the forms the kernels use now meet them everywhere."""
import numpy as np
import pytest
import torch

import step_cases as SC

ids = lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c)


def ce_errs(case):
    ref = SC.ce_reference(*case)
    lg, y = SC.ce_inputs(*case)
    v64 = float(ref.r64["loss"])
    return (SC.err_of("loss", SC.ce_loss_old_formula32(lg, y), v64), SC.err_of("loss", SC.ce_loss_log1p_formula32(lg, y), v64),
            ref.bar("loss", SC.LOSS_CAP))


@pytest.mark.parametrize("case", SC.CE_CASES, ids=ids)
def test_ce_case_conditions(case):
    regime, C, M, ignore = case
    ref = SC.ce_reference(*case)
    lg, y = SC.ce_inputs(*case)
    assert tuple(lg.shape) == (M, C) and lg.dtype == torch.float32 and bool(((y == SC.IGNORE) | ((y >= 0) & (y < C))).all())
    v64 = float(ref.r64["loss"])
    # the margins stop at 20 because float64 log_softmax itself degrades beyond: its loss still agrees with the log1p form to 1e-9
    assert SC.err_of("loss", SC.ce_loss_log1p64(lg, y), v64) <= 1e-9
    assert ref.bar("loss", SC.LOSS_CAP) <= SC.LOSS_CAP and ref.bar("dlogits", SC.GRAD_CAP) <= SC.GRAD_CAP
    if regime == "random":
        assert ref.cond["loss"] <= 1e-6
    if regime == "late":
        assert 1e-2 <= v64 <= 1.0
    if regime == "dead":
        assert C >= 2 and not bool((y == C - 1).any()) and bool((lg[:, C - 1] == SC.DEAD_LOGIT).all())
    if regime == "equal":
        assert v64 == pytest.approx(np.log(C), rel=1e-12) and bool((lg == lg[:, :1]).all())
    if ignore == "all":
        assert np.isnan(v64) and not ref.r64["dlogits"].any()
    if ignore == "all_but_one":
        assert int((y != SC.IGNORE).sum()) == 1
    if ignore == "seventh":
        assert bool((y[::7] == SC.IGNORE).all()) and not ref.r64["dlogits"][::7].any()


def test_ce_cases_cover_the_sweep():
    by = lambda i: {c[i] for c in SC.CE_CASES}
    assert by(0) == set(SC.CE_REGIMES) and by(1) == set(SC.CE_CLASSES) and by(2) == set(SC.CE_M) and by(3) == set(SC.CE_IGNORES)
    for C in SC.CE_CLASSES:
        assert {"random", "right12"} <= {c[0] for c in SC.CE_CASES if c[1] == C}, C
    for regime in SC.CE_REGIMES:
        assert {2, 3} <= {c[1] for c in SC.CE_CASES if c[0] == regime}, regime
    assert max(SC.CE_M) > SC.CE_GRID_FWD and sorted(SC.CE_M)[-2] > SC.CE_GRID_COUNT and max(SC.CE_M) <= 600_000
    assert len(SC.CE_SHIFT_PAIRS) >= 3
    for a, b in SC.CE_SHIFT_PAIRS:                                # + 100 is exact: the float64 losses of a pair agree to 1e-12
        assert a in SC.CE_CASES and b in SC.CE_CASES
        (la, ya), (lb, yb) = SC.ce_inputs(*a), SC.ce_inputs(*b)
        assert torch.equal(lb.double(), la.double() + 100.0) and torch.equal(ya, yb)
        va, vb = float(SC.ce_reference(*a).r64["loss"]), float(SC.ce_reference(*b).r64["loss"])
        assert abs(va - vb) <= 1e-12 * abs(va)


@pytest.mark.parametrize("case", SC.CE_CASES, ids=ids)
def test_ce_bars_can_fail(case):
    """(mx + logf(se)) - l[y] misses the bar on every right12 case and meets it on every random one; log1pf(rest) + (mx - l[y]) meets
    it on every case."""
    regime, C, M, ignore = case
    old, new, bar = ce_errs(case)
    print(f"| ce {ids(case)} | loss | {SC.ce_reference(*case).cond['loss']:.1e} | {bar:.1e} | old {old:.1e} | log1p {new:.1e} |")
    assert new <= bar
    if regime == "random":
        assert old <= bar
    if regime == "right12" and C > 1 and ignore != "all":         # one class: the loss is exactly 0 either way
        assert old > bar


@pytest.mark.parametrize("path", SC.EVAL_PATHS, ids=ids)
def test_eval_case_conditions(path):
    loss, C, storage = path
    for regime in SC.CE_REGIMES:
        ref = SC.eval_reference(regime, loss, C)
        v64 = float(ref.r64["loss"])
        assert np.isfinite(v64) and v64 >= 0.0
        if regime == "random":
            assert ref.cond["loss"] <= 1e-6
        if regime == "late":
            assert 1e-2 <= v64 <= 1.0
        for lg, y in SC.eval_inputs(regime, loss, C):
            assert bool((y == SC.IGNORE).any()) == (loss == "ce")
    assert loss == "ce" or C <= 8


@pytest.mark.parametrize("run", SC.ADAM_RUNS, ids=ids)
def test_adam_case_conditions_and_bars_can_fail(run):
    """1.f - powf(beta, step) and 1.f - beta from fp32 betas miss the bar on the small-weight chains and meet it at the magnitudes of
    test_adam_kernel_exact; the double-on-host forms meet it on every case."""
    tag, n = run
    ref = SC.adam_reference(tag, n)
    p = SC.adam_inputs(tag, n)[0]
    assert float(np.abs(ref.r64["p"]).max()) > 1e-6
    cap = SC.opt_cap()
    if SC.ADAM_CASES[tag][0] != "existing":                       # rounding p cannot reach the bar
        assert float(p.abs().max()) <= 2.0 ** -7 and float(np.abs(p.double().numpy() + ref.r64["p"]).max()) <= 2.0 ** -7
    old, new = SC.adam_formula32(tag, n, "powf32"), SC.adam_formula32(tag, n, "double")
    for k in ("p", "m", "v"):
        eo, en, bar = SC.err_of(k, old[k], ref.r64[k]), SC.err_of(k, new[k], ref.r64[k]), ref.bar(k, cap)
        print(f"| adam {tag} n={n} | {k} | {ref.cond[k]:.1e} | {bar:.1e} | old {eo:.1e} | double {en:.1e} |")
        assert bar <= cap and en <= bar, (k, en, bar)
        if tag == "existing_s7":
            assert eo <= bar, (k, eo, bar)
    if tag in SC.ADAM_SMALL:
        assert SC.err_of("p", old["p"], ref.r64["p"]) > ref.bar("p", cap)


def test_adam_cap_and_unchanged_case():
    assert 1e-5 < SC.opt_cap() < 1e-3                             # 5e-7 against a largest update of about 1e-2
    ref = SC.adam_reference("unchanged", 257)
    assert not ref.r64["p"].any() and not ref.r64["m"].any() and not ref.r64["v"].any()
    assert {n for t, n in SC.ADAM_RUNS if t == "small_s1"} == set(SC.OPT_SIZES) and max(SC.OPT_SIZES) > SC.OPT_GRID
    assert {t for t, _ in SC.ADAM_RUNS} == set(SC.ADAM_CASES)


@pytest.mark.parametrize("run", SC.SGD_RUNS, ids=ids)
def test_sgd_case_conditions(run):
    tag, n = run
    ref = SC.sgd_reference(tag, n)
    p = SC.sgd_inputs(tag, n)[0]
    assert float(np.abs(ref.r64["p"]).max()) > 1e-6 and float(p.abs().max()) <= 2.0 ** -7
    assert ("buf" in ref.r64) == (SC.SGD_CASES[tag][0] != 0.0)
    assert ref.bar("p", SC.opt_cap()) <= SC.opt_cap()
    assert {t for t, _ in SC.SGD_RUNS} == set(SC.SGD_CASES) and {n for t, n in SC.SGD_RUNS if t == "m0.9_wd0.0001"} == set(SC.OPT_SIZES)
