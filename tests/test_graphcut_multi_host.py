"""CPU tier of the K-label graph cut: the numpy oracle (tests/graphcut_multi_oracle.py) that the GPU tier compares the kernels with is
itself checked here -- every single move against an independent max flow (scipy) of a differently built representation of that move,
the final labelling against brute force and the expansion bound on small grids, K = 2 against the binary oracle, energy bookkeeping and
convergence far inside the default cycle cap -- together with the API surface that needs no device."""
import itertools

import numpy as np
import pytest

import graphcut_cases as GC
import graphcut_multi_cases as MC
import graphcut_multi_oracle as GMO
import graphcut_oracle as GO
import mgunet
from test_graphcut_host import scipy_cut

HOST_CASES = ["n1k3", "k1", "tiepair", "zero16", "grid5x7", "grid16", "grid33x31", "random200", "init16", "binary16"]


def independent_move(L, alpha, N, coo, U, ce):
    """The move "x_i = 1: node i takes alpha" in a representation that shares nothing with the kernel's: the pair term
    t(0,0) = A, t(0,1) = B, t(1,0) = C, t(1,1) = 0 is written once from either end and the two forms are added, which gives TWICE
    the function with the same arc capacity B + C - A in both directions and x-coefficients C - A - B (lower end), B - A - C (higher
    end).  -> the labelling of the largest minimiser, by scipy's max flow and a residual reverse BFS."""
    U = np.clip(np.asarray(U, np.int64), 0, GMO.CAP_MAX)
    u, v = np.asarray(coo[0], np.int64), np.asarray(coo[1], np.int64)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    pos = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(u, v))}
    w = np.array([min(max(int(ce[pos[(int(a), int(b))]]), 0), GMO.CAP_MAX) for a, b in zip(lo, hi)], np.int64) if len(u) else np.zeros(0, np.int64)
    a, b = L[lo], L[hi]
    A, B, C = w * (a != b), w * (a != alpha), w * (alpha != b)
    coef = 2 * (U[:, alpha] - U[np.arange(N), L])          # cost of x_i = 1 minus cost of x_i = 0, doubled like the pair terms
    once = u < v
    np.add.at(coef, lo[once], (C - A - B)[once])
    np.add.at(coef, hi[once], (B - A - C)[once])
    ct, cs = np.maximum(coef, 0), np.maximum(-coef, 0)     # paid when the node is foreground (takes alpha) / background
    _, fg = scipy_cut(N, coo, cs, ct, B + C - A)
    return np.where(fg != 0, alpha, L)


@pytest.mark.parametrize("name", HOST_CASES)
def test_every_move_equals_an_independent_solve(name):
    N, coo, U, ce, _ = MC.multi_case(name)
    got = MC.expanded(name)
    assert got["trace"], name
    for before, alpha, proposed, accepted in got["trace"]:
        assert np.array_equal(independent_move(before, alpha, N, coo, U, ce), proposed), (name, alpha)
        e0, e1 = GMO.energy_multi(before, coo, U, ce), GMO.energy_multi(proposed, coo, U, ce)
        assert e1 <= e0 and accepted == (e1 < e0), (name, alpha, e0, e1)   # a move never raises E; equal cost is dropped


@pytest.mark.parametrize("name", HOST_CASES + ["grid64x32"])
def test_energy_bookkeeping_and_convergence_far_inside_the_cycle_cap(name):
    N, coo, U, ce, init = MC.multi_case(name)
    got = MC.expanded(name)
    K = U.shape[1]
    assert got["converged"] == 1 and got["energy"] == GMO.energy_multi(got["labels"], coo, U, ce)
    assert got["moves"] <= 8 * K, (name, got["moves"], K)             # a quarter of the default cap of 32 cycles
    assert got["accepted"] == sum(t[3] for t in got["trace"]) and got["moves"] == len(got["trace"])
    assert got["labels"].max() < K
    assert got["energy"] <= GMO.energy_multi(GMO.start_labels(U, init), coo, U, ce)
    assert not any(t[3] for t in got["trace"][-K:])                   # the K closing idle moves
    print(f"{name}: K={K} moves={got['moves']} accepted={got['accepted']} rounds={got['rounds']} energy={got['energy']}")


def test_expansion_against_brute_force_on_2x3_grids():
    coo = GC.grid_edges(2, 3)
    N, K = 6, 3
    all_L = np.array(list(itertools.product(range(K), repeat=N)), np.int64)
    u, v = coo
    met = 0
    for seed in range(30):
        rng = np.random.RandomState(100 + seed)
        U = rng.randint(0, 3000, (N, K)).astype(np.int64)
        w = rng.randint(0, 2500, coo.shape[1] // 2)
        ce = GMO.pairs(coo, np.zeros(coo.shape[1]))                   # the pair list, to give both arcs of a pair one weight
        cap = np.zeros(coo.shape[1], np.int64)
        cap[ce[3]], cap[ce[4]] = w, w
        got = GMO.expand(N, coo, U, cap)
        en = U[np.arange(N), all_L].sum(1) + (cap[None, :] * ((all_L[:, u] != all_L[:, v]) & (u < v)[None, :])).sum(1)
        best = int(en.min())
        assert got["converged"] == 1 and best <= got["energy"] <= 2 * best, (seed, got["energy"], best)
        met += got["energy"] == best
        L = got["labels"].astype(np.int64)
        for alpha in range(K):                                        # no single further expansion lowers it: all 2^6 subsets
            for mask in range(1 << N):
                cand = np.where((mask >> np.arange(N)) & 1, alpha, L)
                assert GMO.energy_multi(cand, coo, U, cap) >= got["energy"]
    print(f"expansion met the brute-force optimum on {met} of 30 grids")


def test_two_labels_from_the_background_start_are_the_binary_cut():
    N, coo, U, ce, init = MC.multi_case("binary16")
    got, ref = MC.expanded("binary16"), GC.solved("grid16")
    assert np.array_equal(got["labels"], ref["labels"]) and got["energy"] == ref["flow"]
    assert (got["moves"], got["accepted"]) == (4, 1)                  # alpha = 0 idle, alpha = 1 is the cut, two idle moves close
    N2, coo2, cs, ct, ce2 = GC.solver_case("grid16")
    assert GMO.energy_multi(ref["labels"], coo, U, ce) == GO.energy(ref["labels"], coo2, cs, ct, ce2)   # E(L) is E(S) for K = 2


def test_strict_accept_and_start_rules():
    got = MC.expanded("tiepair")
    assert got["labels"].tolist() == [0, 1] and (got["energy"], got["moves"], got["accepted"]) == (4, 2, 0)
    assert [t[2].tolist() for t in got["trace"]] == [[0, 0], [1, 1]]  # what the moves proposed: equal cost, dropped
    z = MC.expanded("zero16")
    assert not z["labels"].any() and (z["energy"], z["moves"], z["accepted"], z["rounds"]) == (0, 3, 0, 0)
    assert all((t[2] == t[1]).all() for t in z["trace"])              # every move proposed all-alpha: the largest foreground
    assert MC.expanded("n1k3")["labels"].tolist() == [1] and MC.expanded("n1k3")["energy"] == 3
    assert MC.expanded("k1")["moves"] == 1 and not MC.expanded("k1")["labels"].any()
    U = np.array([[5, 2, 2], [1, 1, 9]])
    assert GMO.start_labels(U).tolist() == [1, 0]                     # the lowest label on ties
    assert GMO.start_labels(U, np.array([2, 3])).tolist() == [2, 0] and GMO.start_labels(U, np.array([255, 1])).tolist() == [1, 1]
    N, coo, Ug, ce, _ = MC.multi_case("grid33x31")
    capped = GMO.expand(N, coo, Ug, ce, max_cycles=1)
    assert capped["converged"] == 0 and capped["moves"] == 5
    assert GMO.energy_multi(capped["labels"], coo, Ug, ce) == capped["energy"] <= GMO.energy_multi(GMO.start_labels(Ug), coo, Ug, ce)
    rcap = GMO.expand(N, coo, Ug, ce, max_rounds=1)                   # a move whose solve hits the round cap ends the loop
    assert (rcap["converged"], rcap["moves"], rcap["accepted"]) == (0, 1, 0) and np.array_equal(rcap["labels"], GMO.start_labels(Ug))


def test_label_costs_oracle_and_the_float32_condition():
    counts = np.array([[3, 1, 0], [0, 0, 0], [0, 256, 0]])
    want = [[-np.log(4 / 7), -np.log(2 / 7), -np.log(1 / 7)], [-np.log(1 / 3)] * 3, [-np.log(1 / 259), -np.log(257 / 259), -np.log(1 / 259)]]
    assert np.array_equal(GMO.label_costs(counts), np.rint(np.array(want) * 1024).astype(np.int64))
    two = np.array([[3, 1], [0, 0]])
    assert np.array_equal(GMO.label_costs(two)[:, 1], GO.quant(-np.log(GO.prior_from_counts(two, 1))))   # K = 2: the binary prior
    p = np.array([[0.0, 1.0, 0.5, 1e-7]], np.float32)
    big = int(np.rint(-np.log(1e-6) * 1024))
    assert GMO.label_costs(p).tolist() == [[big, 0, 710, big]]
    assert GMO.label_costs(p, unit=2.0 ** 17)[0, 0] == 1 << 20         # the ceiling
    # the inputs of the GPU tier's probability test: a float32 evaluation differs from float64 by at most one unit in at most 1 of 1000
    prob = MC.class_maps(12, 10, 5, 33)[0]
    f32 = np.minimum(np.rint(np.maximum(-np.log(np.clip(prob, np.float32(1e-6), np.float32(1))) * np.float32(1024), 0)), 1 << 20).astype(np.int64)
    d = np.abs(f32 - GMO.label_costs(prob))
    assert d.max() <= 1 and (d != 0).mean() <= 1e-3, (int(d.max()), float((d != 0).mean()))


def test_api_surface_without_a_device():
    import torch
    for name in ("graph_cut_multi", "label_costs", "cut_energy_multi", "MultiCut"):
        assert hasattr(mgunet, name) and name in mgunet.__all__
    assert callable(mgunet.MinCutRefinement.solve_multi) and callable(mgunet.MinCutRefinement.refine_patches_multi)
    args = (None, None, None, mgunet.MinCutRefinement(), None, None)
    assert mgunet.MinGraphUNetE2E(*args, num_segments=3, partition="expansion").partition == "expansion"
    assert mgunet.MinGraphUNetE2E(*args, num_segments=2, partition="expansion").num_segments == 2
    with pytest.raises(ValueError, match="num_segments >= 2"):
        mgunet.MinGraphUNetE2E(*args, num_segments=1, partition="expansion")
    with pytest.raises(ValueError, match="num_segments must be 2"):      # the binary partition keeps its rule
        mgunet.MinGraphUNetE2E(*args, num_segments=3, partition="mincut")
    from mgunet import _lib
    protos = _lib.parse_header()
    assert {"mgu_graphcut_label_costs", "mgu_graphcut_expand", "mgu_graphcut_energy_multi"} <= set(protos)
    assert len(protos["mgu_graphcut_expand"][1]) == 23 and protos["mgu_graphcut_expand"][2]
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # a CPU tensor is refused, not computed
        mgunet.label_costs(torch.full((2, 3), 0.3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mgunet.graph_cut_multi(ei, torch.zeros((2, 3), dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError):
        mgunet.graph_cut_multi(ei, [[0, 1]], torch.zeros(2, dtype=torch.int32))
