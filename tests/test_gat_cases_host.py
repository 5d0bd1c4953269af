"""The cases of tests/gat_cases.py, looked at without a GPU: every graph, batch and layer shape has the property it is there for (a
later edit cannot silently turn a hub into an ordinary row), the kernel instance each (shape, batch) pair selects is the one the
case is meant to launch (the launchers' conditions restated in plain Python), the two ill-conditioned cases meet their conditions
on the oracle alone, and the dev32 / devfx / bar table -- the base of every bar in tests/test_gpu_gat_f64.py -- is printed under -s.
A bar above 1e-3 would mean a case that tests nothing: refused."""
import numpy as np
import pytest
import torch

import gat_cases as GC
from graph_branch_cases import DUP, HUB_IN, HUB_OUT, LOOP


def csr_rowptr(name):
    ei, gp, _ = GC.layout(name)
    ind = np.bincount(ei[1].numpy(), minlength=gp[-1])
    return np.concatenate([[0], np.cumsum(ind)]), ind, gp


def segments(name):
    """(first row, edges, in-degrees of the rows) of every 4-row CSR segment of gat_aggregate_kernel."""
    rp, ind, gp = csr_rowptr(name)
    N = gp[-1]
    return [(j0, int(rp[min(j0 + 4, N)] - rp[j0]), ind[j0:j0 + 4]) for j0 in range(0, N, 4)]


def show(what, ref):
    for name in ref.r64:
        bar = ref.bar(name)
        print(f"| {what} | {name} | {ref.dev32[name]:.1e} | {ref.devfx[name]:.1e} | {bar:.1e} |")
        assert np.isfinite(bar) and bar <= 1e-3, (what, name, bar)


def test_ladder_general_and_spur_degrees():
    ei = GC.ladder_graph().numpy()
    ind = np.bincount(ei[1], minlength=GC.LADDER_N)
    assert ei.dtype == np.int64 and ei.min() >= 0 and ei.max() < GC.LADDER_N
    assert tuple(ind[:16]) == (0, 1, 3, 4, 5, 7, 8, 9, 12, 16, 17, 63, 64, 65, 129, 2)
    assert ind[GC.LADDER_LONE] == 64 and not ind[GC.LADDER_LONE - 3:GC.LADDER_LONE].any() and not ind[GC.LADDER_LONE + 1:GC.LADDER_LONE + 4].any()
    assert int(ind.sum()) == 405 + 64 and np.any(np.diff(ei[1]) < 0)                     # arbitrary order: not sorted by target
    # every boundary of the 4-slot, 8-slot and 64-id batches and of TRIP = 4 and 8: one below, at, one above
    for b in (4, 8, 16, 64):
        assert {b - 1, b, b + 1} <= set(ind.tolist()) or b == 16 and {16, 17} <= set(ind.tolist()), b
    assert 129 in ind and 129 > 2 * 64 and -(-129 // 8) == 17 and -(-129 // 4) == 33      # third trip of the base += 64 loop; 17 / 33 trips
    g = GC.batch("general")[0][0].numpy()
    gin, gout = np.bincount(g[1], minlength=101), np.bincount(g[0], minlength=101)
    assert gin[HUB_IN] >= 70 and gout[HUB_OUT] >= 70 and -(-int(gin[HUB_IN]) // 4) >= 18
    assert int(((g[0] == LOOP) & (g[1] == LOOP)).sum()) >= 2 and int(((g[0] == DUP[0]) & (g[1] == DUP[1])).sum()) >= 4
    assert gout[100] == 0 and gin[100] > 0 and gin[99] == 0 and gout[99] > 0 and gin[98] == 0 and gout[98] == 0
    s = GC.spur_graph().numpy()
    assert np.bincount(s[1], minlength=GC.SPUR_N)[GC.SPUR_HUB] == 70 and s.shape[1] == 97
    t = GC.tiny_graph().numpy()
    assert t.shape == (2, 1) and not t.any()


@pytest.mark.parametrize("name", ["dense", "big", "sparse", "many"])
def test_batch_properties(name):
    ei, gp, parts = GC.layout(name)
    N, E = gp[-1], ei.shape[1]
    ind, outd = GC.degrees(name)
    segs = segments(name)
    print(f"{name}: N {N}, E {E}, graphs {len(parts)}, max in-degree {ind.max()}, max out-degree {outd.max()}, graph_ptr {gp}")
    if name != "many":
        assert N % 4 and N % 32                                                          # a ragged last segment and a ragged last tile
        assert any(b % 4 for b in gp[1:-1]) and all(b % 32 for b in gp[1:-1])            # segments and 32-node tiles straddle graphs
    if name in ("dense", "big"):
        assert E > 4 * N                                                                 # the DENSE instance at HF <= 256
        k = [i for i, p in enumerate(parts) if p[0].shape[1] == 0]
        assert k and 0 < k[0] < len(parts) - 1 and parts[k[0] - 1][0].shape[1] and parts[k[0] + 1][0].shape[1]   # edgeless graph in the middle
        assert outd.max() >= 70                                                          # gatb_source_kernel: a source with 70 out-edges
        assert GC.lone_masked_edge(name) is not None
    if name == "sparse":
        assert E <= 4 * N and ind.max() == 70
        assert sum(1 for j0, ne, d in segs if d.max() <= 4 and ne) >= 10                 # fast-path segments (4 x 4 batch)
    if name == "big":
        nb = GC.da_row_blocks(N)
        rows = -(-N // nb)
        assert nb == 3 and N - 2 * rows not in (0, rows)                                 # three row blocks, the last one ragged
    else:
        assert GC.da_row_blocks(N) == 1
    if name == "many":
        assert len(parts) * 32 > 256                                                     # gmax_buffer regrows at 32 heads
    # gat_aggregate_kernel: a segment of exactly 64 edges (ids held in the wave), one above (ids reloaded per row), a row with a
    # second trip of the base += 64 loop, and a segment under 64 edges that leaves the fast path by a row of more than 8
    assert any(ne == 64 for _, ne, _ in segs) or name == "sparse"
    assert any(ne > 64 for _, ne, _ in segs) and ind.max() > 64
    assert any(ne <= 64 and d.max() > 8 for _, ne, d in segs) or name == "sparse"
    assert any(ne > 64 and ((d > 0) & (d < 64)).any() for _, ne, d in segs)                  # shorter rows inside a long segment
    # gat_fused2_kernel: more than three trips of TRIP = 8
    assert ind.max() > 3 * 8


def test_kernel_instances():
    """Which instance each (shape, batch) pair launches."""
    for name in ("dense", "sparse"):
        ei, gp, _ = GC.layout(name)
        N, E = gp[-1], ei.shape[1]
        for s in GC.FUSED_SHAPES:
            assert GC.fused_applicable(*s, E), s
        got = {s: GC.aggregate_instance(s[1], s[2], N, E) for s in GC.GATHER_SHAPES}
        dense = name == "dense"
        assert got == {(32, 4, 64): (1, dense), (36, 3, 20): (1, dense), (16, 8, 32): (1, dense), (4, 1, 4): (1, dense), (32, 1, 256): (1, dense),
                       (32, 8, 64): (2, False), (64, 6, 64): (2, False), (32, 32, 32): (4, False), (48, 5, 128): (4, False)}, name
    assert sorted(GC.FUSED_SHAPES) == sorted((a, h, b) for a, b in ((32, 32), (32, 64), (64, 64)) for h in (1, 2, 4))
    # not fused-applicable whatever the environment says: only (32, 4, 64) of the gather family needs MGU_NO_GAT_FUSED
    assert [s for s in GC.GATHER_SHAPES if GC.fused_applicable(*s, 1)] == [(32, 4, 64)]
    # 32 * 8 * 64 / 4 = 128 quads fill NCH 2, 6 * 64 / 4 = 96 fill it partly; 256 fill NCH 4, 160 partly; heads at the limit
    assert [h * f // 4 for _, h, f in GC.GATHER_SHAPES[5:]] == [128, 96, 256, 160] and GC.GATHER_SHAPES[7][1] == 32
    assert (16, 8, 32) in GC.GATHER_SHAPES and 8 > 4 and 8 * 32 <= 256                    # heads > 4 at HF <= 256: no fast path
    assert (32, 1, 256) in GC.GATHER_SHAPES and 4 * (256 // 4) > 64                      # fast-path head mean over RB * qh = 256 quads
    for Fin, H, Fh in GC.BWD_SHAPES + [GC.WIDE_HUB[1:4], GC.PLATEAU[1:4]]:
        assert H * Fh <= 256 and Fin % 4 == 0 and Fh % 4 == 0
    assert any(H > 1 and (Fh // 4) & (Fh // 4 - 1) for _, H, Fh in GC.BWD_SHAPES)        # head_sum at a non-power-of-two qh, several heads


def test_masks():
    for name, shape in (("dense", (32, 4, 64)), ("big", (36, 3, 20))):
        ei = GC.layout(name)[0]
        for concat in (0, 1):
            X, W, a, R, em, om = GC.inputs(name, *shape, concat)
            k = GC.lone_masked_edge(name)
            assert int((ei[1] == ei[1, k]).sum()) == 1 and not em[:, k].any()            # a degree-1 row whose only edge is masked out
            assert set(np.unique(em.numpy())) == set(np.unique(om.numpy())) == {0.0, np.float32(1.0 / 0.7)}
            assert 0.2 < float((em == 0).float().mean()) < 0.4 and 0.2 < float((om == 0).float().mean()) < 0.4
            assert em.shape == (shape[1], ei.shape[1]) and om.shape == R.shape
    params, shapes, heads, X, R, masks = GC.module_inputs("net")
    assert X.shape[1] % 4 and all(Fh % 4 for _, Fh, _, _ in shapes)                      # every width is padded
    assert not masks[0][0][:, GC.lone_masked_edge("general")].any()


def test_plateau_ties_and_max_gradient():
    b, Fin, H, Fh, xs, ws = GC.PLATEAU
    ei = GC.layout(b)[0]
    A = ei[1] < GC.PLATEAU_A
    assert torch.equal(A, ei[0] < GC.PLATEAU_A) and int(A.sum()) == 40                   # edges run only A -> A and B -> B
    X = GC.inputs(b, Fin, H, Fh, 1)[0]
    assert all(torch.equal(X[i], X[0]) for i in range(GC.PLATEAU_A))                      # bit-identical rows
    for dt in (torch.float64, torch.float32):
        e = GC.edge_scores(b, Fin, H, Fh, dt)
        for h in range(H):
            ties = e[h] == e[h].max()
            assert int(ties.sum()) == int(A.sum()) and torch.equal(ties, A), (dt, h)     # every A -> A edge ties, in either precision
            lo, hi = float(e[h][A].min() - e[h][~A].max()), float(e[h][A].max() - e[h][~A].min())
            assert 20.0 <= lo <= hi <= 26.0, (dt, h, lo, hi)
    max_gradient_matters(GC.PLATEAU)


def test_wide_hub_max_gradient():
    b, Fin, H, Fh, xs, ws = GC.WIDE_HUB
    e = GC.edge_scores(b, Fin, H, Fh, torch.float32, xs, ws)
    print("wide_hub: arg-max ties per head", (e == e.max(1, keepdim=True).values).sum(1).tolist())
    max_gradient_matters(GC.WIDE_HUB)


def max_gradient_matters(case):
    """The float64 gradient with the max detached is at least 50 bars from the true one in dX, dW or da: a backward that drops or
    misplaces the max term cannot pass."""
    b, Fin, H, Fh, xs, ws = case
    for concat in (0, 1):
        ref = GC.reference(b, Fin, H, Fh, concat, "grad", xs, ws)
        det = GC.detached_max_gradients(b, Fin, H, Fh, concat, xs, ws)
        far = {k: GC.rel_err(det[k], ref.r64[k]) / ref.bar(k) for k in ("dX", "dW", "da")}
        print(f"{b} concat {concat}: max-detached gradient, in bars: " + ", ".join(f"{k} {v:.0f}" for k, v in far.items()))
        assert max(far.values()) >= 50.0, far
        show(f"{b} concat {concat}", ref)


def test_bar_table():
    for name in ("dense", "sparse"):
        for fam, shapes in (("fused", GC.FUSED_SHAPES), ("gather", GC.GATHER_SHAPES)):
            for s in shapes:
                for concat in (0, 1):
                    show(f"eval {fam} {s} `{name}` concat {concat}", GC.reference(name, *s, concat, "eval"))
    show("eval gather (32, 32, 32) `many` concat 1", GC.reference("many", 32, 32, 32, 1, "eval"))
    show("eval fused (32, 4, 32) `many` concat 0", GC.reference("many", 32, 4, 32, 0, "eval"))
    for name, shapes in (("dense", GC.BWD_SHAPES), ("big", GC.BIG_SHAPES)):
        for s in shapes:
            for concat in (0, 1):
                for mode in ("grad", "train"):
                    show(f"{mode} {s} `{name}` concat {concat}", GC.reference(name, *s, concat, mode))
    for kind in ("layer", "net"):
        show(f"module {kind}", GC.module_reference(kind))
