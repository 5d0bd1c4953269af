"""The cases of tests/graph_branch_cases.py, looked at without a GPU: every graph has the properties the kernels' edge loops are
tested for, the float64 oracle is consistent with its analytic gradient on them, no segment sits near the kernels' association
threshold, and the dev32 table (deviation of the fp32 oracle from the float64 oracle, the base of every bar in
tests/test_gpu_graph_branch_f64.py) is printed under -s.  A dev32 above 1e-4 would mean an ill-conditioned case: refused."""
import numpy as np
import pytest
import torch

import graph_branch_cases as GC
import mgunet_oracle as O


def show(what, ref):
    for name, dev in ref.dev32.items():
        print(f"| {what} | {name} | {dev:.1e} | {ref.bar(name):.1e} |")
        assert dev < 1e-4, (what, name, dev)


@pytest.mark.parametrize("tag", list(GC.NCUT_CASES))
def test_graph_properties(tag):
    N, D, K, E, _, _, seed = GC.NCUT_CASES[tag]
    ei = GC.general_graph(N, E, seed).numpy()
    src, tgt = ei
    assert ei.dtype == np.int64 and ei.shape[0] == 2 and ei.shape[1] <= E and ei.min() >= 0 and ei.max() < N
    assert np.array_equal(ei[:, :146], GC.general_graph(N, E, seed).numpy()[:, :146])
    out_deg, in_deg = np.bincount(src, minlength=N), np.bincount(tgt, minlength=N)
    assert np.all(src[:70] == GC.HUB_OUT) and out_deg[GC.HUB_OUT] >= 70          # the hub rows survive the drop rule whole
    assert np.all(tgt[70:140] == GC.HUB_IN) and in_deg[GC.HUB_IN] >= 70
    assert np.all(ei[:, 140:142] == GC.LOOP) and int(((src == GC.LOOP) & (tgt == GC.LOOP)).sum()) >= 2
    assert np.all(src[142:146] == GC.DUP[0]) and np.all(tgt[142:146] == GC.DUP[1])
    assert int(((src == GC.DUP[0]) & (tgt == GC.DUP[1])).sum()) >= 4
    assert out_deg[N - 1] == 0 and in_deg[N - 1] > 0                              # no out-edges
    assert in_deg[N - 2] == 0 and out_deg[N - 2] > 0                              # no in-edges
    assert out_deg[N - 3] == 0 and in_deg[N - 3] == 0                             # isolated
    spread = max(int(out_deg[g:g + 16].max() - out_deg[g:g + 16].min()) for g in range(0, N, 16))
    assert spread > 60                                                            # the 16-lane kernel's wave-wide trip count
    print(f"{tag}: E' = {ei.shape[1]}, hub out {out_deg[GC.HUB_OUT]}, hub in {in_deg[GC.HUB_IN]}, mean out-degree "
          f"{ei.shape[1] / N:.1f}, widest out-degree spread in a 16-node group {spread}")


@pytest.mark.parametrize("tag", list(GC.NCUT_CASES))
def test_ncut_oracle_gradient_consistency_threshold_and_dev32(tag):
    ei, X, L, R, K, unaligned = GC.ncut_inputs(tag)
    ref = GC.ncut_prob_reference(tag)
    # float64 autograd of normalized_cut_loss == the analytic normalized_cut_loss_grad
    dP, dX = O.normalized_cut_loss_grad(X.double(), ei, torch.softmax(L, dim=1).double(), K, gloss=GC.GLOSS)
    assert GC.rel_err(dP, ref.r64["dP"]) <= 1e-12 and GC.rel_err(dX, ref.r64["dX"]) <= 1e-12
    # the kernels compare the association with 1e-8 in fp32: every segment is far from that on either side
    assoc = GC.ncut_assoc64(tag)
    assert np.all((assoc > 1e-3) | (assoc < 1e-12)), assoc
    assert int((assoc < 1e-12).sum()) == (1 if tag == "skip" else 0)
    w = ref.r64["w"]
    print(f"{tag}: edge weights in [{w.min():.3f}, {w.max():.3f}], association in [{assoc.min():.2e}, {assoc.max():.2e}], "
          f"max|dX| {np.abs(ref.r64['dX']).max():.2e}")
    show(f"ncut probabilities `{tag}`", ref)
    lref = GC.ncut_logit_reference(tag)
    show(f"ncut logits `{tag}`", lref)
    if tag == "skip":
        assert abs(float(lref.r64["loss"]) - GC.ncut_loss_without(tag, GC.SKIPPED)) <= 1e-12 * float(lref.r64["loss"])
        assert np.abs(lref.r64["dL_skip"]).max() < 1e-20       # effectively zero, and the bar applies to it as a tensor of its own
    if tag == "k1":
        assert not lref.r64["dL"].any() and not lref.r64["dX"].any() and np.all(lref.r64["soft"] == 1.0)


@pytest.mark.parametrize("case", GC.FEATCONS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_feature_consistency_cases(case):
    fu, fg, y, margin = GC.featcons_inputs(case)
    assert torch.equal(fu[0, 0], fg[0, 0])
    hinge, ones = GC.featcons_hinge_share(case)
    print(f"{case}: hinge active on {100 * hinge:.0f} % of rows, y == 1 on {100 * ones:.0f} %")
    assert 0.05 < hinge < 0.6 and 0.2 < ones < 0.8             # both branches of the loss carry weight
    show(f"feature consistency {case}", GC.featcons_reference(case))


def test_dice_tv_pool_cases():
    for case in GC.DICE_CASES:
        ref = GC.dice_reference(case)
        show(f"dice {case}", ref)
        if case[1] == 1:
            assert not ref.r64["grad"].any() and float(ref.r64["value"]) == 0.0
    ref = GC.dice_raw_reference()
    show(f"dice accumulate {GC.DICE_RAW}", ref)
    g = np.abs(GC.dice_reference(GC.DICE_RAW).r64["grad"]).max() * GC.DICE_RAW_SCALE * GC.DICE_RAW_SCALE_DEV
    assert 0.1 < g / (3 * GC.DICE_RAW_PREFILL) < 10, g       # increment and prefill of one magnitude: a wrong increment shows
    for kind in ("nhwc", "slice"):
        show(f"tv {kind}", GC.tv_reference(kind))
    for case in GC.POOL_CASES:
        B, Np, D, K = case
        feats, lab, empty = GC.pool_inputs(case)
        ref = GC.pool_reference(case)
        counts = np.stack([np.bincount(lab.reshape(B, Np)[b].numpy(), minlength=K) for b in range(B)])
        assert lab.min() >= 0 and lab.max() < K
        for b in range(B):
            assert counts[b, empty[b]] == 0 and not ref.r64["mean"][b * K + empty[b]].any()
        assert (counts > 0).sum() >= B                          # and a non-empty segment in every image
        show(f"region pool {case}", ref)


def test_fuse_and_csr_cases():
    for case in GC.FUSE_CASES:
        B, H, W, K, Cu, D = case
        fu, emb, lab, nph, npw = GC.fuse_inputs(case)
        assert (fu is None) == (Cu == 0) and lab.min() >= 0 and lab.max() < K and lab.numel() == B * nph * npw
        assert tuple(GC.fuse_reference(case).shape) == (B, Cu + D, H, W)
    for N, E in GC.CSR_CASES:
        ei = GC.csr_edges(N, E)
        assert tuple(ei.shape) == (2, E) and (E == 0 or (int(ei.min()) >= 0 and int(ei.max()) < N))
