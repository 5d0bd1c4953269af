"""The optimizer step whose decisions stay on the device (csrc/optim.hip): mgu_grad_norm, mgu_optim_step, mgu_grad_accumulate and what
mgunet.Trainer / FlatAdam build on them (AdamW, norm clipping, skip of a non-finite step, weight EMA, accumulation).

Cases, float64 references and bars are tests/optim_cases.py: the sum of squares within (n + 2) 2^-53 of math.fsum of the exact
squares, every chain quantity within min(4 * cond + 2^-22, opt_cap()) of torch's own float64 run (clip_grad_norm_ + Adam / AdamW /
SGD + the EMA recurrence).  Everything else here is exact: counts, bits run to run, bits whatever the buffers' alignment, bits of
a skipped step, launch counts."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

import mgunet
import mgunet_oracle as O
import optim_cases as OC
from mgunet import _lib

pytestmark = pytest.mark.gpu

ids = lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c)
NEW_KERNELS = {"grad_norm_partial_kernel": 1, "optim_control_kernel": 1, "optim_update_kernel": 1}
STEP_KERNELS = set(NEW_KERNELS) | {"adam_kernel", "sgd_kernel"}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b) -> bool:
    return torch.equal(bits(a), bits(b))


def new_ctrl(dev, fill=0):
    return torch.full((_lib.OPTIM_CTRL_BYTES // 8,), fill, device=dev, dtype=torch.int64)


def record(ctrl) -> dict:
    c = ctrl.cpu().contiguous()
    f64, f32, i32 = c.view(torch.float64), c.view(torch.float32), c.view(torch.int32)
    return {"step": int(c[0]), "skipped": int(c[1]), "sumsq": float(f64[2]), "norm": float(f64[3]), "scale": float(f32[8]),
            "bc1": float(f32[9]), "bc2_sqrt": float(f32[10]), "ema_d": float(f32[11]), "apply": int(i32[12]), "nonfinite": int(i32[13])}


def at_offset(t, dev, offset):
    """a device copy of t that starts `offset` floats past a 16-byte boundary (None stays None)"""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 4, device=dev, dtype=torch.float32)
    v = buf[offset:offset + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * offset
    return v


def make_desc(kind, lr=None, wd=0.0, momentum=0.0, grad_scale=1.0, max_norm=0.0, skip=False, ema=0.0, warm=False):
    return _lib.OptimDesc(OC.KIND_CODE[kind], OC.lr_of(kind) if lr is None else lr, OC.ADAM_BETAS[0], OC.ADAM_BETAS[1], OC.ADAM_EPS, wd,
                          momentum, grad_scale, max_norm, int(skip), ema, int(warm))


def optim_step(dev, d, p, g, m, v, e, ctrl, ctx=None):
    _lib.call("mgu_optim_step", dev, C.byref(d), p, g, m, v, e, ctrl, p.numel(), ctx=ctx)


def launches(ctx, fn) -> dict:
    _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 1), ctx.handle)
    try:
        fn()
        return {k["name"]: k["launches"] for k in _lib.read_kernel_stats(ctx)}
    finally:
        _lib.check(_lib.lib().mgu_profile_enable(ctx.handle, 0), ctx.handle)


# ---- mgu_grad_norm ------------------------------------------------------------------------------------------------------------------
def grad_norm(dev, g, gs=0.125, fill=0):
    ctrl = new_ctrl(dev, fill)
    _lib.call("mgu_grad_norm", dev, g, g.numel(), gs, ctrl)
    return ctrl.cpu()


@pytest.mark.parametrize("run", OC.NORM_RUNS, ids=ids)
def test_grad_norm(cuda, run):
    content, n = run
    g = OC.norm_input(content, n)
    ref, bar = OC.norm_reference(content, n), OC.sumsq_bar(n)
    first = grad_norm(cuda, g.to(cuda), fill=0x0101010101010101)
    r = record(first)
    err = OC.sumsq_err(r["sumsq"], ref)
    print(f"| grad_norm {content} n={n} | sumsq | {bar:.1e} | {err:.1e} |")
    assert err <= bar, (r["sumsq"], ref)
    assert abs(r["norm"] - 0.125 * math.sqrt(r["sumsq"])) <= 2.0 ** -51 * r["norm"] and r["nonfinite"] == 0
    untouched = new_ctrl("cpu", 0x0101010101010101)                                      # the call writes sumsq, norm, nonfinite alone
    keep = torch.ones(16, dtype=torch.bool)
    keep[4:8] = False
    keep[13] = False
    assert torch.equal(first.view(torch.int32)[keep], untouched.view(torch.int32)[keep])
    assert torch.equal(first, grad_norm(cuda, g.to(cuda), fill=0x0101010101010101))      # bitwise, run to run
    for offset in (1, 2, 3):                                                             # ... and wherever the buffer starts
        shifted = record(grad_norm(cuda, at_offset(g, cuda, offset)))
        assert (np.float64(shifted["sumsq"]).view(np.uint64), shifted["nonfinite"]) == (np.float64(r["sumsq"]).view(np.uint64), 0), offset


def test_grad_norm_counts_non_finite_elements_exactly(cuda):
    n = OC.OPT_GRID + 1
    chunk, blocks = int(_lib.lib().mgu_grad_norm_chunk(n)), int(_lib.lib().mgu_grad_norm_blocks(n))
    assert chunk % 4 == 0 and (blocks - 1) * chunk < n <= blocks * chunk and blocks > 2
    base = OC.norm_input("normal", n)
    spots = {0: float("inf"), n - 1: float("nan"), chunk - 1: float("nan"), chunk: float("-inf"), 2 * chunk - 1: float("inf"),
             2 * chunk: float("nan"), n - 2: float("inf")}
    for offset in (0, 1):
        for where, value in spots.items():
            g = base.clone()
            g[where] = value
            assert record(grad_norm(cuda, at_offset(g, cuda, offset)))["nonfinite"] == 1, (where, offset)
        g = base.clone()
        for where, value in spots.items():
            g[where] = value
        assert record(grad_norm(cuda, at_offset(g, cuda, offset)))["nonfinite"] == len(spots), offset
    for m in (1, 5, 257):                                                                # below one quad, one workgroup
        g = OC.norm_input("normal", m)
        g[0], g[m - 1] = float("inf"), float("nan")
        assert record(grad_norm(cuda, g.to(cuda)))["nonfinite"] == (1 if m == 1 else 2), m


# ---- mgu_optim_step: chains ---------------------------------------------------------------------------------------------------------
def run_chain(dev, tag, n, offsets=(0, 0, 0, 0, 0), max_norm=None):
    """The case's chain on the device from a zeroed record.  offsets: floats past a 16-byte boundary of p, g, m, v, ema."""
    kind, mom, wd, gs, clip, ema, warm, mag, bad = OC.CASES[tag]
    p0, grads, case_max = OC.inputs(tag, n)
    d = make_desc(kind, wd=wd, momentum=mom, grad_scale=gs, max_norm=case_max if max_norm is None else max_norm, skip=bad is not None, ema=ema,
                  warm=warm)
    p = at_offset(p0, dev, offsets[0])
    m = at_offset(torch.zeros(n), dev, offsets[2]) if (kind != "sgd" or mom) else None
    v = at_offset(torch.zeros(n), dev, offsets[3]) if kind != "sgd" else None
    e = at_offset(p0, dev, offsets[4]) if ema else None
    ctrl = new_ctrl(dev)
    for g in grads:
        optim_step(dev, d, p, at_offset(g, dev, offsets[1]), m, v, e, ctrl)
    out = {"p": p.cpu()}
    if kind == "sgd":
        if mom:
            out["buf"] = m.cpu()
    else:
        out["m"], out["v"] = m.cpu(), v.cpu()
    if ema:
        out["ema"] = e.cpu()
    return out, record(ctrl)


@pytest.mark.parametrize("run", OC.RUNS, ids=ids)
def test_optim_chain(cuda, run):
    tag, n = run
    ref, cap = OC.reference(tag, n), OC.opt_cap()
    p0 = OC.inputs(tag, n)[0]
    got, rec = run_chain(cuda, tag, n)
    what = f"optim {tag} n={n}"
    for k in ref.r64:
        ref.check(k, OC.update_of(got[k], p0) if k == "p" else got[k], cap, what)
    bad = OC.CASES[tag][8]
    assert (rec["step"], rec["skipped"], rec["apply"], rec["nonfinite"]) == (OC.OPT_STEPS, int(bad is not None), 1, 0)
    coef = OC.clip_coefs(tag, n)[-1]
    assert abs(rec["scale"] - OC.CASES[tag][3] * coef) <= 2.0 ** -22 * abs(rec["scale"])
    assert abs(rec["bc1"] - (1.0 - OC.ADAM_BETAS[0] ** OC.OPT_STEPS)) <= 2.0 ** -23
    again, rec2 = run_chain(cuda, tag, n)                                                # bitwise, run to run
    assert rec == rec2 and all(same_bits(got[k], again[k]) for k in got)


@pytest.mark.parametrize("tag", ["adamw_clip", "adam_clip", "sgd_m0.9_clip", "sgd_m0_clip"])
def test_chain_bits_do_not_depend_on_alignment(cuda, tag):
    """p, g, m, v and ema on a common offset (16-byte body after a peeled head) and on different ones (element by element)"""
    n = 100003
    want, rec = run_chain(cuda, tag, n)
    for offsets in ((1, 1, 1, 1, 1), (3, 3, 3, 3, 3), (0, 1, 2, 3, 0), (2, 0, 0, 0, 0)):
        got, rec2 = run_chain(cuda, tag, n, offsets)
        assert rec == rec2 and all(same_bits(want[k], got[k]) for k in want), offsets


# ---- mgu_optim_step: exact properties -----------------------------------------------------------------------------------------------
def test_a_norm_below_max_norm_changes_no_bit(cuda):
    for n in (257, 100003):
        clipped, rec = run_chain(cuda, "adamw_far", n)
        plain, rec0 = run_chain(cuda, "adamw_far", n, max_norm=0.0)
        assert OC.inputs("adamw_far", n)[2] > rec["norm"] > 0.0 and rec == rec0
        assert all(same_bits(clipped[k], plain[k]) for k in clipped)


@pytest.mark.parametrize("kind,mom", [("adam", 0.0), ("adamw", 0.0), ("sgd", 0.9), ("sgd", 0.0)])
def test_a_skipped_step_keeps_every_bit_and_does_not_count(cuda, kind, mom):
    n = 100003
    p0, grads, _ = OC.inputs("adam_clip", n)
    d = make_desc(kind, wd=1e-2, momentum=mom, max_norm=0.05, skip=True, ema=0.9)
    bad = grads[0].clone()
    bad[n - 1] = float("nan")

    def chain(gs):
        p, m, v, e, ctrl = p0.to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda), p0.to(cuda), new_ctrl(cuda)
        states = []
        for g in gs:
            optim_step(cuda, d, p, g.to(cuda), m if kind != "sgd" or mom else None, v if kind != "sgd" else None, e, ctrl)
            states.append(([t.cpu() for t in (p, m, v, e)], record(ctrl)))
        return states

    (skipped, rec_s), (after, rec_a) = chain([bad, grads[0]])
    zeros = torch.zeros(n)
    assert all(same_bits(a, b) for a, b in zip(skipped, (p0, zeros, zeros, p0)))
    assert (rec_s["step"], rec_s["skipped"], rec_s["apply"], rec_s["nonfinite"]) == (0, 1, 0, 1)
    (fresh, rec_f), = chain([grads[0]])
    assert all(same_bits(a, b) for a, b in zip(after, fresh))                            # the next finite step is step 1
    assert (rec_a["step"], rec_a["skipped"], rec_a["apply"]) == (1, 1, 1) and rec_a["bc1"] == rec_f["bc1"] and rec_a["scale"] == rec_f["scale"]
    (_, rec_n), = chain([bad.clone().fill_(float("inf"))])                               # every element: the count is n
    assert rec_n["nonfinite"] == n and rec_n["apply"] == 0


def test_without_skip_a_non_finite_gradient_steps_and_counts(cuda):
    """nothing is promised about the values; the call returns, the step counts and the record says what it saw"""
    n = 257
    g = OC.norm_input("normal", n)
    g[3] = float("nan")
    p, m, v = (torch.zeros(n, device=cuda) for _ in range(3))
    ctrl = new_ctrl(cuda)
    optim_step(cuda, make_desc("adam", max_norm=1.0), p, g.to(cuda), m, v, None, ctrl)
    rec = record(ctrl)
    assert (rec["step"], rec["skipped"], rec["apply"], rec["nonfinite"]) == (1, 0, 1, 1)


def test_no_ema_buffer_is_needed_without_ema(cuda):
    n = 257
    p0, grads, _ = OC.inputs("adam", n)
    p, m, v, ctrl = p0.to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda), new_ctrl(cuda)
    optim_step(cuda, make_desc("adamw", wd=1e-2, ema=0.0), p, grads[0].to(cuda), m, v, None, ctrl)
    assert record(ctrl)["step"] == 1 and not same_bits(p, p0)


@pytest.mark.parametrize("kind,mom", [("adam", 0.0), ("adamw", 0.0), ("sgd", 0.9), ("sgd", 0.0)])
def test_zero_gradient_on_zero_state_changes_nothing(cuda, kind, mom):
    """g = 0 on zero state without decay: the update is 0 / (0 + eps), and p, m and v keep their bits (clip on: 0 * coef is 0)"""
    for n in (257, OC.OPT_GRID + 1):
        p0 = OC.inputs("adam", n)[0]
        for max_norm in (0.0, 1.0):
            p, m, v, ctrl = p0.to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda), new_ctrl(cuda)
            for _ in range(2):
                optim_step(cuda, make_desc(kind, momentum=mom, max_norm=max_norm), p, torch.zeros(n, device=cuda), m, v, None, ctrl)
            assert same_bits(p, p0) and not bool(m.any()) and not bool(v.any()) and record(ctrl)["step"] == 2


# ---- mgu_grad_accumulate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, OC.OPT_GRID + 1])
def test_grad_accumulate(cuda, n):
    gs = [(OC._normal(f"ocase/acc/g{i}", (n,), 9) * 1e-2).float() for i in range(3)]
    for off_a, off_g in ((0, 0), (1, 1), (0, 3)):
        acc = at_offset(torch.full((n,), float("nan")), cuda, off_a)
        want = None
        for i, g in enumerate(gs):
            _lib.call("mgu_grad_accumulate", cuda, acc, at_offset(g, cuda, off_g), n, int(i == 0))
            want = g.clone() if i == 0 else want + g                                     # fp32, one rounding per element and call
            assert same_bits(acc, want), (n, i, off_a, off_g)


# ---- launch counts ------------------------------------------------------------------------------------------------------------------
def test_optim_step_is_three_launches_whatever_the_options(cuda):
    ctx = _lib.context(cuda)
    for n in (1, OC.OPT_GRID + 1):
        p, g, m, v, e = (torch.zeros(n, device=cuda) for _ in range(5))
        for kind, clip, skip, ema in itertools.product(("adam", "adamw", "sgd"), (0.0, 1.0), (False, True), (0.0, 0.9)):
            d = make_desc(kind, momentum=0.9, max_norm=clip, skip=skip, ema=ema)
            ctrl = new_ctrl(cuda)
            got = launches(ctx, lambda: optim_step(cuda, d, p, g, m, v, e if ema else None, ctrl))
            assert got == NEW_KERNELS, (n, kind, clip, skip, ema, got)
        got = launches(ctx, lambda: _lib.call("mgu_grad_norm", cuda, g, n, 1.0, new_ctrl(cuda)))
        assert got == {"grad_norm_partial_kernel": 1, "optim_control_kernel": 1}, (n, got)
        got = launches(ctx, lambda: _lib.call("mgu_grad_accumulate", cuda, p, g, n, 0))
        assert got == {"grad_accumulate_kernel": 1}, (n, got)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(cuda):
    ctx = _lib.context(cuda)
    n = 16
    p, g, m, v, e = (torch.zeros(n, device=cuda) for _ in range(5))
    ctrl = new_ctrl(cuda)

    def rejected(d, ema=e, **kw):
        def call():
            with pytest.raises(ValueError):
                optim_step(cuda, d, kw.get("p", p), kw.get("g", g), kw.get("m", m), kw.get("v", v), ema, ctrl)
        assert launches(ctx, call) == {}

    bad_kind = make_desc("adam")
    for k in (-1, 3):
        bad_kind.kind = k
        rejected(bad_kind)
    rejected(make_desc("adam", max_norm=-1.0))
    rejected(make_desc("adam", max_norm=float("nan")))
    for decay in (-0.1, 1.0, 1.5):
        rejected(make_desc("adam", ema=decay))
    rejected(make_desc("adam", ema=0.9), ema=None)
    rejected(make_desc("adamw"), v=None)
    rejected(make_desc("sgd", momentum=0.9), m=None)
    with pytest.raises(ValueError):
        _lib.call("mgu_optim_step", cuda, None, p, g, m, v, e, ctrl, n)
    with pytest.raises(ValueError):
        _lib.call("mgu_optim_step", cuda, C.byref(make_desc("adam")), p, g, m, v, e, ctrl, 0)
    with pytest.raises(ValueError):
        _lib.call("mgu_grad_norm", cuda, g, 0, 1.0, ctrl)
    with pytest.raises(ValueError):
        _lib.call("mgu_grad_norm", cuda, g, n, float("inf"), ctrl)
    with pytest.raises(ValueError):
        _lib.call("mgu_grad_accumulate", cuda, p, p, n, 0)
    assert record(ctrl)["step"] == 0 and not bool(p.any())


# ---- Trainer and FlatAdam -----------------------------------------------------------------------------------------------------------
CFG, SHAPE = (3, 2, 8, 2), (2, 3, 32, 32)
OPTS = dict(optimizer="adamw", lr=1e-3, weight_decay=1e-2, max_grad_norm=0.5, ema_decay=0.9)


def build(seed, dev):
    m = mgunet.UNet(*CFG)
    m.load_state_dict(O.make_unet_params(*CFG, seed=seed))
    return m.to(dev)


@pytest.fixture(scope="module")
def batch(cuda):
    x = torch.from_numpy(O.formula_normal("optim/x", SHAPE, seed=61)).to(cuda)
    y = torch.from_numpy(O.formula_labels("optim/y", (SHAPE[0], SHAPE[2], SHAPE[3]), CFG[1], seed=62)).to(cuda)
    return x, y


def test_trainer_steps_are_mgu_optim_step_on_its_buffers(cuda, batch, tmp_path):
    x, y = batch
    model = build(71, cuda)
    tr = mgunet.Trainer(model, **OPTS)
    n = tr.flat.numel()
    p, m, v, e, ctrl = tr.flat.clone(), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda), tr.flat.clone(), new_ctrl(cuda)
    assert same_bits(tr.ema, tr.flat)                                                    # the EMA starts as a copy of the parameters
    d = make_desc("adamw", lr=OPTS["lr"], wd=OPTS["weight_decay"], max_norm=OPTS["max_grad_norm"], ema=OPTS["ema_decay"])
    for step in range(3):
        tr.train_step(x, y)
        optim_step(cuda, d, p, tr.grad, m, v, e, ctrl)                                   # the same gradient, by hand
        assert torch.equal(ctrl, tr.ctrl), step
        assert all(same_bits(a, b) for a, b in zip((p, m, v, e), (tr.flat, tr.exp_avg, tr.exp_avg_sq, tr.ema))), step
    assert float(tr.grad_norm) == record(ctrl)["norm"] > 0.0 and tr.grad_norm.is_cuda and tr.grad_norm.dtype == torch.float64
    assert (tr.applied_steps(), tr.skipped_steps()) == (3, 0)

    sd = tr.optimizer_state_dict()                                                       # torch.optim.AdamW's layout
    params = [q for _, q in model.named_parameters()]
    opt = torch.optim.AdamW(params, lr=0.5)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["weight_decay"] == OPTS["weight_decay"] and opt.param_groups[0]["lr"] == OPTS["lr"]
    assert float(opt.state[params[0]]["step"]) == 3.0
    assert same_bits(torch.cat([opt.state[q]["exp_avg_sq"].reshape(-1) for q in params]), tr.exp_avg_sq)

    path = str(tmp_path / "ck.pt")                                                       # the checkpoint carries the EMA and the step count
    tr.save_checkpoint(path, 1, 0.5)
    ck = torch.load(path, map_location="cpu")
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "loss", "ema_state_dict"}
    assert set(ck["ema_state_dict"]) == set(ck["model_state_dict"])
    other = mgunet.Trainer(build(72, cuda), **OPTS)
    other.load_checkpoint(path)
    assert same_bits(other.ema, tr.ema) and same_bits(other.flat, tr.flat) and same_bits(other.exp_avg, tr.exp_avg)
    assert (other.applied_steps(), other.step_count) == (3, 3)
    tr.train_step(x, y)
    other.train_step(x, y)
    assert same_bits(other.flat, tr.flat) and same_bits(other.ema, tr.ema) and torch.equal(other.ctrl, tr.ctrl)


def test_ema_weights_swap_in_and_back(cuda, batch):
    x, y = batch
    model = build(73, cuda)
    tr = mgunet.Trainer(model, **OPTS)
    for _ in range(2):
        tr.train_step(x, y)
    flat, ema = tr.flat.clone(), tr.ema.clone()
    model.eval()
    with torch.no_grad():
        live = model(x)[0].clone()
        with tr.ema_weights():
            assert same_bits(tr.flat, ema) and same_bits(tr.ema, flat)
            averaged = model(x)[0].clone()
        back = model(x)[0].clone()
    assert not same_bits(averaged, live) and same_bits(back, live)
    assert same_bits(tr.flat, flat) and same_bits(tr.ema, ema)
    sd = tr.ema_state_dict()
    name, q = next(iter(model.named_parameters()))
    assert same_bits(sd[name].reshape(-1), ema[:q.numel()]) and sd[name].shape == q.shape
    bn = next(k for k in sd if k.endswith("running_mean"))
    assert same_bits(sd[bn], model.state_dict()[bn])                                     # buffers are the live model's
    tr.train_step(x, y)                                                                  # training continues
    assert tr.applied_steps() == 3
    with pytest.raises(RuntimeError):
        mgunet.Trainer(build(73, cuda)).ema_state_dict()


def test_accumulate_adds_the_gradients_and_steps_every_kth_call(cuda, batch):
    x, y = batch
    single = mgunet.Trainer(build(74, cuda))
    halves = []
    for b in range(2):
        single.forward_backward(x[b:b + 1], y[b:b + 1])
        halves.append(single.grad.clone())
    model = build(74, cuda)
    tr = mgunet.Trainer(model, accumulate=2)
    ctx = model._context(cuda)
    start = tr.flat.clone()
    got = launches(ctx, lambda: tr.train_step(x[0:1], y[0:1]))
    assert got.get("grad_accumulate_kernel") == 1 and not (STEP_KERNELS & set(got)), got
    assert same_bits(tr.flat, start) and same_bits(tr.acc, halves[0])
    got = launches(ctx, lambda: tr.train_step(x[1:2], y[1:2]))
    assert got.get("grad_accumulate_kernel") == 1 and all(got.get(k) == 1 for k in NEW_KERNELS), got
    assert same_bits(tr.acc, halves[0] + halves[1]) and tr.applied_steps() == 1 and not same_bits(tr.flat, start)
    p, m, v, ctrl = start.clone(), torch.zeros_like(start), torch.zeros_like(start), new_ctrl(cuda)              # the same step by hand:
    optim_step(cuda, make_desc("adam", lr=1e-3, wd=1e-4, grad_scale=0.5), p, halves[0] + halves[1], m, v, None, ctrl)   # Adam on the sum / 2
    assert same_bits(p, tr.flat)


def test_a_non_finite_batch_is_skipped(cuda, batch):
    x, y = batch
    model = build(75, cuda)
    tr = mgunet.Trainer(model, skip_nonfinite=True)
    tr.train_step(x, y)
    flat, m, v = tr.flat.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone()
    bad = x.clone()
    bad[1, 2, 5, 7] = float("inf")
    tr.train_step(bad, y)
    assert same_bits(tr.flat, flat) and same_bits(tr.exp_avg, m) and same_bits(tr.exp_avg_sq, v)
    assert (tr.applied_steps(), tr.skipped_steps(), tr.step_count) == (1, 1, 2)
    assert int(tr.optimizer_state_dict()["state"][0]["step"]) == 1                       # the applied steps, not the attempts


def test_default_trainer_and_flat_adam_step_as_before(cuda, batch, monkeypatch):
    """With every option at its default the step is the mgu_adam_step / mgu_sgd_step call it was.  Those two entry points make no
    profiling records (tests/test_gpu_bench_contract.py pins the records of a default train step, and adam_kernel is not among them),
    so the entry points a step calls are read off _lib.call and the records only have to hold none of the new kernels."""
    x, y = batch
    called, real = [], _lib.call

    def spy(name, *a, **kw):
        called.append(name)
        return real(name, *a, **kw)

    monkeypatch.setattr(_lib, "call", spy)
    new = set(NEW_KERNELS) | {"grad_accumulate_kernel"}
    for optimizer, entry in (("adam", "mgu_adam_step"), ("sgd", "mgu_sgd_step")):
        model = build(76, cuda)
        tr = mgunet.Trainer(model, optimizer=optimizer)
        assert tr.ctrl is None and tr.ema is None and tr.acc is None and not tr.device_step
        before = tr.flat.clone()
        del called[:]
        got = launches(model._context(cuda), lambda: tr.train_step(x, y))
        steps = [c for c in called if c in ("mgu_adam_step", "mgu_sgd_step", "mgu_optim_step", "mgu_grad_norm", "mgu_grad_accumulate")]
        assert steps == [entry] and got and not new & set(got) and not same_bits(tr.flat, before), (steps, got)
        with pytest.raises(RuntimeError):
            tr.applied_steps()
    lin = torch.nn.Linear(7, 5).to(cuda)
    fa = mgunet.FlatAdam([lin])
    del called[:]
    got = launches(_lib.context(cuda), lambda: fa.step())
    assert called == ["mgu_adam_step"] and not new & set(got) and fa.ctrl is None


def test_flat_adam_options(cuda):
    torch.manual_seed(3)
    lin = torch.nn.Linear(7, 5).to(cuda)
    fa = mgunet.FlatAdam([lin], lr=1e-3, weight_decay=1e-2, decoupled=True, max_grad_norm=0.1, skip_nonfinite=True, ema_decay=0.9, ema_warmup=True)
    n = fa.flat.numel()
    p, m, v, e, ctrl = fa.flat.clone(), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda), fa.flat.clone(), new_ctrl(cuda)
    d = make_desc("adamw", lr=1e-3, wd=1e-2, max_norm=0.1, skip=True, ema=0.9, warm=True)
    xs = torch.randn(3, 4, 7, device=cuda)
    for step in range(3):
        fa.zero_grad()
        lin(xs[step]).square().sum().backward()
        got = launches(_lib.context(cuda), lambda: fa.step())
        assert got == NEW_KERNELS
        optim_step(cuda, d, p, fa.grad, m, v, e, ctrl)
        assert torch.equal(ctrl, fa.ctrl) and same_bits(p, fa.flat) and same_bits(e, fa.ema) and same_bits(lin.weight.reshape(-1), p[:35])
    assert fa.applied_steps() == 3 and record(ctrl)["ema_d"] == float(np.float32(min(0.9, 4.0 / 13.0)))
    fa.grad.fill_(float("nan"))
    fa.step()
    assert (fa.applied_steps(), fa.skipped_steps()) == (3, 1) and same_bits(p, fa.flat)


def test_trainer_argument_errors(cuda):
    model = build(77, cuda)
    for kw in (dict(accumulate=0), dict(accumulate=1.5), dict(comm="rccl", accumulate=2), dict(max_grad_norm=-1.0), dict(ema_decay=1.0),
               dict(optimizer="rmsprop")):
        with pytest.raises(ValueError):
            mgunet.Trainer(model, **kw)
    with pytest.raises(ValueError):
        mgunet.FlatAdam([model], ema_decay=-0.5)
