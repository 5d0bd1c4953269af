"""The graph-branch kernels beyond the patch graph against float64: csrc/ncut.hip (the fallback kernel, more than one column trip,
every backward register, hubs, self-loops, duplicate edges, nodes without edges), the auxiliary-loss kernels of csrc/losses.hip at
widths and class counts the fixtures do not have, csrc/region.hip at every thread layout, and mgu_csr_transpose_device directly.

Cases, references and the bar are tests/graph_branch_cases.py: err = max|got - ref64| / max|ref64| with no floor in the
denominator, bar = max(4 * dev32, 16 * eps32), dev32 = the deviation of the oracle run in fp32 from the oracle run in float64,
computed here on the CPU.  Where ref64 is identically zero the kernel's result is exactly zero.  NOTES.md ("Graph-branch float64
bars") carries dev32, the bar and the measured error of every line these tests print under -s."""
import numpy as np
import pytest
import torch

import graph_branch_cases as GC
import mgunet
import mgunet_oracle as O
from mgunet import _lib
from mgunet.gat import coo_to_csr_device

pytestmark = pytest.mark.gpu

NCUT_TAGS = list(GC.NCUT_CASES)


def features(X, cuda, unaligned):
    Xd = X.to(cuda)
    if unaligned:
        Xd = GC.unaligned_view(Xd)
    assert Xd.is_contiguous() and Xd.data_ptr() % 16 == (4 if unaligned else 0)
    return Xd.requires_grad_(True)


def nhwc_stored(x):
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize("tag", NCUT_TAGS)
def test_ncut_probabilities_leaf(cuda, tag):
    """normalized_cut_loss with the soft assignments as the leaf, upstream factor 2.5: loss, dP, dX, the per-edge weights."""
    ei, X, L, _, K, unaligned = GC.ncut_inputs(tag)
    ref = GC.ncut_prob_reference(tag)
    mc = mgunet.MinCutRefinement()
    eid = ei.to(cuda)
    P0 = torch.softmax(L, dim=1).to(cuda)

    def run(view):
        Xd, P = features(X, cuda, view), P0.clone().requires_grad_(True)
        loss = mc.normalized_cut_loss(Xd, eid, P, K)
        (GC.GLOSS * loss).backward()
        return loss.detach(), P.grad, Xd.grad, Xd

    loss, dP, dX, Xd = run(unaligned)
    what = f"ncut probabilities `{tag}`"
    ref.check("loss", loss, what=what)
    ref.check("dP", dP, what=what)
    ref.check("dX", dX, what=what)
    ref.check("w", mc.compute_edge_weights_for_ncut(Xd.detach(), eid), what=what)
    if tag == "skip":     # alpha = beta = 0 for the skipped segment: no term of its column survives
        assert not ref.r64["dP"][:, GC.SKIPPED].any() and float(dP[:, GC.SKIPPED].abs().max()) == 0.0
    # a second backward on fresh leaves gives the same bytes: both gradients are gathers, the forward's sums meet in doubles
    loss2, dP2, dX2, _ = run(unaligned)
    assert torch.equal(loss2, loss) and torch.equal(dP2, dP) and torch.equal(dX2, dX)
    if unaligned:         # the same values in an aligned tensor take the 16-lane kernel: both against float64
        what += " aligned"
        loss_a, dP_a, dX_a, _ = run(False)
        ref.check("loss", loss_a, what=what)
        ref.check("dP", dP_a, what=what)
        ref.check("dX", dX_a, what=what)


@pytest.mark.parametrize("tag", NCUT_TAGS)
def test_ncut_logits_leaf(cuda, tag):
    """MinCutRefinement.forward with the logits as the leaf and a side loss on the returned soft assignments (gsoft_dev and the
    softmax backward): loss, soft, dlogits, dX, hard labels."""
    ei, X, L, R, K, unaligned = GC.ncut_inputs(tag)
    ref = GC.ncut_logit_reference(tag)
    mc = mgunet.MinCutRefinement()
    eid = ei.to(cuda)
    Xd, Ld = features(X, cuda, unaligned), L.to(cuda).requires_grad_(True)
    loss, soft = mc(Xd, eid, K, lambda x, e: Ld)
    (loss + GC.SIDE * (soft * R.to(cuda)).sum()).backward()
    what = f"ncut logits `{tag}`"
    ref.check("loss", loss.detach(), what=what)
    ref.check("soft", soft.detach(), what=what)
    ref.check("dL", Ld.grad, what=what)
    ref.check("dX", Xd.grad, what=what)
    # hard labels = argmax wherever the float64 soft assignment decides it by more than 1e-5
    s64 = ref.r64["soft"]
    top = np.sort(s64, axis=1)
    clear = (top[:, -1] - top[:, -2] > 1e-5) if K > 1 else np.ones(len(s64), dtype=bool)
    hard = mc.last_hard_labels.cpu().numpy()
    assert hard.dtype == np.int64 and clear.sum() >= 0.9 * len(s64)
    assert np.array_equal(hard[clear], s64.argmax(1)[clear])
    if tag == "skip":
        # the loss is the loss with that segment left out, and its gradient column is the float64 one (about 1e-26) to the bar
        without = GC.ncut_loss_without(tag, GC.SKIPPED)
        assert abs(float(loss.detach()) - without) <= ref.bar("loss") * abs(without)
        ref.check("dL_skip", Ld.grad[:, GC.SKIPPED], what=what)
        assert float(Ld.grad[:, GC.SKIPPED].abs().max()) < 1e-20
    if tag == "k1":       # the soft assignment is exactly 1 and nothing reaches the logits
        assert float((soft.detach() - 1.0).abs().max()) == 0.0 and float(Ld.grad.abs().max()) == 0.0


@pytest.mark.parametrize("case", GC.FEATCONS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_feature_consistency_f64(cuda, case):
    fu, fg, y, margin = GC.featcons_inputs(case)
    ref = GC.featcons_reference(case)
    fl = mgunet.FeatureConsistencyLoss(margin=margin)
    yd = y.to(cuda)

    def run(need_u, need_g):
        a, b = fu.to(cuda).requires_grad_(need_u), fg.to(cuda).requires_grad_(need_g)
        v = fl(a, b, yd)
        (GC.FEATCONS_UP * v).backward()
        return v.detach(), a.grad, b.grad

    what = f"feature consistency {case}"
    v, du, dg = run(True, True)
    ref.check("value", v, what=what)
    ref.check("dfu", du, what=what)
    ref.check("dfg", dg, what=what)
    # one gradient alone (the NULL-pointer branches of the kernel): the same bytes as from the run that asks for both
    v_u, du_only, none_g = run(True, False)
    v_g, none_u, dg_only = run(False, True)
    assert none_g is None and none_u is None
    assert torch.equal(du_only, du) and torch.equal(dg_only, dg) and torch.equal(v_u, v) and torch.equal(v_g, v)


def test_dice_backward_wide_classes(cuda):
    for case in GC.DICE_CASES:
        lg, y = GC.dice_inputs(case)
        ref = GC.dice_reference(case)
        for store in ("nchw", "nhwc"):
            l = lg.to(cuda)
            if store == "nhwc":
                l = nhwc_stored(l)
            l.requires_grad_(True)
            v = mgunet.dice_loss(l, y.to(cuda), 1.0)
            v.backward()
            what = f"dice {case} {store}"
            ref.check("value", v.detach(), what=what)
            ref.check("grad", l.grad, what=what)
            if case[1] == 1:
                assert float(l.grad.abs().max()) == 0.0 and float(v.detach()) == 0.0
    mgunet.losses.check_labels(cuda)


def test_dice_backward_accumulate_and_scales_raw_abi(cuda):
    """mgu_dice_loss_backward as the trainer calls it for CE + dice: adding into a destination of pitch 8, grad_scale together
    with grad_scale_dev, the loss written by the same call."""
    B, C, H, W = GC.DICE_RAW
    HW, pitch = H * W, GC.DICE_RAW_PITCH
    lg, y = GC.dice_inputs(GC.DICE_RAW)
    ref = GC.dice_raw_reference()
    lgd, yd = lg.to(cuda).contiguous(), y.to(cuda).contiguous()
    pre = GC.dice_raw_prefill().to(cuda)
    dst = pre.clone()
    assert tuple(dst.shape) == (B * HW, pitch) and dst.is_contiguous() and C <= pitch
    scale_dev = torch.tensor([GC.DICE_RAW_SCALE_DEV], device=cuda, dtype=torch.float32)
    loss = torch.zeros((), device=cuda, dtype=torch.float32)
    _lib.call("mgu_dice_loss_backward", cuda, lgd, yd, B, HW, C, C * HW, HW, 1, 1.0, GC.DICE_RAW_SCALE, scale_dev, dst, HW * pitch, 1,
              pitch, 1, loss)
    ref.check("acc", dst[:, :C], what=f"dice accumulate {GC.DICE_RAW}")
    assert torch.equal(dst[:, C:], pre[:, C:])                  # the pad columns keep their bytes
    fwd = torch.zeros((), device=cuda, dtype=torch.float32)
    _lib.call("mgu_dice_loss", cuda, lgd, yd, B, HW, C, C * HW, HW, 1, 1.0, fwd)
    assert torch.equal(loss, fwd)
    GC.dice_reference(GC.DICE_RAW).check("value", loss, what=f"dice accumulate {GC.DICE_RAW}")
    mgunet.losses.check_labels(cuda)


def test_tv_backward_strided(cuda):
    tv = mgunet.TVLoss(GC.TV_WEIGHT)
    x = nhwc_stored(GC.tv_inputs("nhwc").to(cuda)).requires_grad_(True)
    assert x.stride(1) == 1 and not x.is_contiguous()
    v = tv(x)
    (g,) = torch.autograd.grad(GC.TV_UP * v, x)
    ref = GC.tv_reference("nhwc")
    ref.check("value", v.detach(), what="tv nhwc")
    ref.check("grad", g, what="tv nhwc")
    assert g.stride() == x.stride()                             # NHWC-stored in, NHWC-stored out
    xs = GC.tv_slice(GC.tv_inputs("slice").to(cuda)).detach().requires_grad_(True)
    assert tuple(xs.shape) == GC.TV_SHAPE and not xs.is_contiguous() and xs.stride(2) != xs.shape[3]
    v = tv(xs)
    (g,) = torch.autograd.grad(GC.TV_UP * v, xs)
    ref = GC.tv_reference("slice")
    ref.check("value", v.detach(), what="tv slice")
    ref.check("grad", g, what="tv slice")


def test_region_mean_pool_layouts(cuda):
    for case in GC.POOL_CASES:
        B, Np, D, K = case
        feats, lab, empty = GC.pool_inputs(case)
        got = mgunet.region_mean_pool(feats.to(cuda), lab.to(cuda), B, K)
        assert tuple(got.shape) == (B * K, D)
        GC.pool_reference(case).check("mean", got, what=f"region pool {case}")
        for b in range(B):
            assert float(got[b * K + empty[b]].abs().max()) == 0.0   # an empty segment keeps a zero row


def test_region_fuse_exact(cuda):
    for case in GC.FUSE_CASES:
        B, H, W, K, Cu, D = case
        fu, emb, lab, nph, npw = GC.fuse_inputs(case)
        got = mgunet.region_fuse(None if fu is None else fu.to(cuda), emb.to(cuda), lab.to(cuda), B, H, W, nph, npw, K)
        assert tuple(got.shape) == (B, Cu + D, H, W)
        assert torch.equal(got.cpu(), GC.fuse_reference(case)), case


def test_csr_transpose_device_bit_exact(cuda):
    for N, E in GC.CSR_CASES:
        rowptr, col = coo_to_csr_device(GC.csr_edges(N, E).to(cuda), N)          # CSR by target: col = sources
        rp = torch.full((N + 1,), -1, dtype=torch.int32, device=cuda)
        eid = torch.full((max(E, 1),), -1, dtype=torch.int32, device=cuda)
        tgt = torch.full((max(E, 1),), -1, dtype=torch.int32, device=cuda)
        _lib.call("mgu_csr_transpose_device", cuda, rowptr, col if E else None, E, N, rp, eid, tgt)
        rowptr_h, col_h = rowptr.cpu().numpy(), col.cpu().numpy()
        assert np.array_equal(tgt.cpu().numpy()[:E], np.repeat(np.arange(N, dtype=np.int32), np.diff(rowptr_h))), (N, E)
        assert np.array_equal(eid.cpu().numpy()[:E], np.argsort(col_h, kind="stable").astype(np.int32)), (N, E)
        want = np.concatenate([[0], np.cumsum(np.bincount(col_h, minlength=N))]).astype(np.int32)
        assert np.array_equal(rp.cpu().numpy(), want), (N, E)
