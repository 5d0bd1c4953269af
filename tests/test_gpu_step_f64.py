"""The kernels every training run reports and applies, against float64 on the logits and weights of a TRAINED network: the
segmentation loss and its gradient (mgu_cross_entropy: ce_count_kernel, ce_fwd_bwd_kernel of csrc/train_kernels.hip), the validation
loss of mgunet.SegmentationEvaluator (mgu_segmentation_eval, csrc/seg_eval.hip: the C == 2 fast path, the register path up to 8
classes, the loop beyond, with and without the dice term) and the optimizer steps (mgu_adam_step, mgu_sgd_step) in chains of three
calls with the state kept on the device.

Cases, references and bars are tests/step_cases.py: bar = min(4 * cond + 2^-22, CAP) with cond the deviation of torch's own fp32 run
of the reference from float64, a loss measured relative to ITSELF, a parameter against its update.  Ignored rows, pad columns and
gradients whose float64 value is identically zero are exact zeros.  NOTES.md ("Loss and optimizer kernels: float64 bars on a trained
network") carries the lines these tests print under -s, and the same lines from the kernels as they were before."""
import numpy as np
import pytest
import torch

import mgunet
import step_cases as SC
from mgunet import _lib

pytestmark = pytest.mark.gpu

ids = lambda c: "-".join(map(str, c)) if isinstance(c, tuple) else str(c)


# ---- mgu_cross_entropy --------------------------------------------------------------------------------------------------------------
def run_ce(cuda, case, scale):
    """(loss, dlogits (M, pitch)) of one mgu_cross_entropy call with grad_scale = scale / M; dlogits starts as NaN."""
    regime, C, M, ignore = case
    lg, y = SC.ce_inputs(*case)
    pitch = (C + 3) // 4 * 4
    dl = torch.full((M, pitch), float("nan"), device=cuda)
    loss = torch.full((1,), -5.0, device=cuda)
    _lib.call("mgu_cross_entropy", cuda, lg.to(cuda), y.to(cuda), M, C, scale / M, dl, loss)
    _lib.call("mgu_sync_check", cuda)
    return float(loss), dl.cpu()


@pytest.mark.parametrize("case", SC.CE_CASES, ids=ids)
def test_cross_entropy_loss_and_gradient(cuda, case):
    regime, C, M, ignore = case
    ref = SC.ce_reference(*case)
    y = SC.ce_inputs(*case)[1]
    what = "ce " + ids(case)
    for scale in SC.CE_SCALES:
        loss, dl = run_ce(cuda, case, scale)
        if scale == SC.CE_SCALES[0]:
            ref.check("loss", np.float64(loss), SC.LOSS_CAP, what)
        else:
            assert SC.err_of("loss", np.float64(loss), ref.r64["loss"]) <= ref.bar("loss", SC.LOSS_CAP)
        ref.check("dlogits", dl[:, :C].double() / scale, SC.GRAD_CAP, f"{what} scale {scale}")
        assert float(dl[:, C:].abs().sum()) == 0.0 and not bool(torch.isnan(dl).any())      # pad columns up to the pitch
        assert float(dl[y == SC.IGNORE].abs().sum()) == 0.0                                  # ignored rows
        if ignore == "all":
            assert np.isnan(loss) and float(dl.abs().sum()) == 0.0
        if C == 1:
            assert loss == 0.0


@pytest.mark.parametrize("pair", SC.CE_SHIFT_PAIRS, ids=lambda p: ids(p[0]))
def test_cross_entropy_does_not_feel_a_shift_of_the_logits(cuda, pair):
    """The float64 losses of right12 and of right12 + 100 agree to 1e-12; the kernel's may differ by the two bars at most."""
    a, b = pair
    ra, rb = SC.ce_reference(*a), SC.ce_reference(*b)
    la, lb = run_ce(cuda, a, 1.0)[0], run_ce(cuda, b, 1.0)[0]
    v64 = float(ra.r64["loss"])
    bar = ra.bar("loss", SC.LOSS_CAP) + rb.bar("loss", SC.LOSS_CAP)
    err = abs(lb - la) / v64
    print(f"| ce {ids(b)} - {ids(a)} | loss shift | {ra.cond['loss'] + rb.cond['loss']:.1e} | {bar:.1e} | {err:.1e} |")
    assert err <= bar, (la, lb, v64)


# ---- the validation loss of SegmentationEvaluator -----------------------------------------------------------------------------------
def host_cm(y, pred, C):
    y, pred = y.reshape(-1).numpy(), pred.reshape(-1).numpy()
    keep = (y >= 0) & (y < C)
    return np.bincount(y[keep] * C + pred[keep], minlength=C * C).reshape(C, C)


def nchw_view(nhwc_host, dev, offset):
    """(B, C, H, W) view of NHWC device storage, shifted by `offset` floats (1: no 16-byte alignment, the generic path for C == 2)."""
    B, H, W, C = nhwc_host.shape
    buf = torch.empty(nhwc_host.numel() + offset, device=dev)
    v = buf[offset:].view(B, H, W, C)
    v.copy_(nhwc_host.to(dev))
    assert (v.data_ptr() % 16 == 0) == (offset == 0)
    return v.permute(0, 3, 1, 2)


@pytest.mark.parametrize("path", SC.EVAL_PATHS, ids=ids)
def test_validation_loss(cuda, path):
    loss, C, storage = path
    offset = {"aligned": 0, "offset1": 1}[storage]
    for regime in SC.CE_REGIMES:
        ref = SC.eval_reference(regime, loss, C)
        batches = SC.eval_inputs(regime, loss, C)
        accs, cm = [], np.zeros((C, C), dtype=np.int64)
        for rep in range(2):
            ev = mgunet.SegmentationEvaluator(C, cuda, loss=loss, dice_smooth=SC.EVAL_DICE_SMOOTH)
            for lg, y in batches:                                                            # three batches of unequal size
                pred = ev.update(nchw_view(lg, cuda, offset), y.to(cuda), return_pred=True)
                if rep == 0:
                    want = torch.argmax(lg.permute(0, 3, 1, 2), 1)
                    assert torch.equal(pred.cpu(), want)
                    cm += host_cm(y, want, C)
            res = ev.compute()
            accs.append(ev.loss_acc.cpu().numpy().copy())
            assert np.array_equal(res["confusion_matrix"], cm)
        ref.check("loss", np.float64(res["loss"]), SC.LOSS_CAP, f"eval {loss} C={C} {storage} {regime}")
        assert accs[0][1] == len(batches)
        assert np.array_equal(accs[0].view(np.uint64), accs[1].view(np.uint64))              # bitwise, run to run


# ---- mgu_adam_step, mgu_sgd_step ----------------------------------------------------------------------------------------------------
def run_adam(cuda, tag, n):
    p, grads, m, v, step, gs, wd = SC.adam_inputs(tag, n)
    dp, dm, dv = (t.clone().to(cuda) for t in (p, m, v))
    for k, g in enumerate(grads):                                                            # the state stays on the device
        _lib.call("mgu_adam_step", cuda, dp, g.to(cuda), dm, dv, n, SC.ADAM_LR, SC.ADAM_BETAS[0], SC.ADAM_BETAS[1], SC.ADAM_EPS, wd,
                  step + k, gs)
    return (p, m, v), (dp.cpu(), dm.cpu(), dv.cpu())


@pytest.mark.parametrize("run", SC.ADAM_RUNS, ids=ids)
def test_adam_chain(cuda, run):
    tag, n = run
    ref, cap = SC.adam_reference(tag, n), SC.opt_cap()
    (p0, _, _), (p, m, v) = run_adam(cuda, tag, n)
    what = f"adam {tag} n={n}"
    ref.check("p", SC.update_of(p, p0), cap, what)
    ref.check("m", m, cap, what)
    ref.check("v", v, cap, what)


def test_adam_zero_gradient_changes_nothing(cuda):
    """g = 0 on zero state without decay: the update is 0 / (0 + eps), and p, m and v keep their bits."""
    for n in (257, SC.OPT_GRID + 1):
        before, after = run_adam(cuda, "unchanged", n)
        for b, a in zip(before, after):
            assert torch.equal(b.view(torch.int32), a.view(torch.int32))


@pytest.mark.parametrize("run", SC.SGD_RUNS, ids=ids)
def test_sgd_chain(cuda, run):
    tag, n = run
    p0, grads, mom, wd = SC.sgd_inputs(tag, n)
    ref, cap = SC.sgd_reference(tag, n), SC.opt_cap()
    dp = p0.clone().to(cuda)
    buf = torch.full((n,), float("nan"), device=cuda) if mom else None                       # the first step copies the gradient into it
    for k, g in enumerate(grads):
        _lib.call("mgu_sgd_step", cuda, dp, g.to(cuda), buf, n, SC.SGD_LR, mom, wd, 1 + k, 1.0)
    what = f"sgd {tag} n={n}"
    ref.check("p", SC.update_of(dp.cpu(), p0), cap, what)
    if mom:
        ref.check("buf", buf.cpu(), cap, what)
