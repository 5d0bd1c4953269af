"""CPU tier of the graph cut: the numpy oracle (tests/graphcut_oracle.py) that the GPU tier compares the kernels with is itself checked
here -- flow and canonical labels against scipy's max flow plus a residual reverse BFS on every solver input, the tie rule, E(labels)
== flow, convergence far inside the default round cap -- together with the API surface that needs no device."""
import numpy as np
import pytest

import graphcut_cases as GC
import graphcut_oracle as GO
import mgunet


def scipy_cut(N, coo, cs, ct, ce):
    """(flow value, labels): labels 1 iff the sink is not reachable from the node in the residual graph of scipy's maximum flow"""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import maximum_flow
    S, T = N, N + 1
    rows = np.concatenate([coo[0], np.full(N, S), np.arange(N)])
    cols = np.concatenate([coo[1], np.arange(N), np.full(N, T)])
    cap = sp.csr_matrix((np.concatenate([ce, cs, ct]).astype(np.int32), (rows, cols)), shape=(N + 2, N + 2))
    res = maximum_flow(cap, S, T)
    resid = (cap - res.flow).tocoo()                      # flow is antisymmetric: reverse arcs get their residual too
    live = resid.data > 0
    ru, rv = resid.row[live], resid.col[live]
    reach = np.zeros(N + 2, bool)
    reach[T] = True
    while True:
        new = reach.copy()
        new[ru[reach[rv]]] = True
        if np.array_equal(new, reach):
            break
        reach = new
    return int(res.flow_value), (~reach[:N]).astype(np.uint8)


@pytest.mark.parametrize("name", GC.SOLVER_CASES)
def test_oracle_equals_scipy_max_flow(name):
    N, coo, cs, ct, ce = GC.solver_case(name)
    got = GC.solved(name)
    flow, labels = scipy_cut(N, coo, cs, ct, ce)
    assert got["converged"] == 1
    assert got["flow"] == flow
    assert np.array_equal(got["labels"], labels)


@pytest.mark.parametrize("name", GC.SOLVER_CASES)
def test_oracle_energy_of_its_labels_is_the_flow_and_rounds_stay_far_inside_the_cap(name):
    N, coo, cs, ct, ce = GC.solver_case(name)
    got = GC.solved(name)
    assert GO.energy(got["labels"], coo, cs, ct, ce) == got["flow"]
    assert got["converged"] == 1 and got["rounds"] <= (8 * N + 64) // 10, got["rounds"]
    for period in (1, 8, 1000):                           # the result does not depend on the relabel period
        other = GO.solve(N, coo, cs, ct, ce, period=period)
        assert other["flow"] == got["flow"] and np.array_equal(other["labels"], got["labels"]) and other["converged"] == 1


def test_tie_path_labels_both_nodes_foreground():
    got = GC.solved("tie")
    assert got["flow"] == 5 and got["labels"].tolist() == [1, 1]
    N, coo, cs, ct, ce = GC.solver_case("tie")
    assert [GO.energy(l, coo, cs, ct, ce) for l in ([0, 0], [1, 0], [1, 1])] == [5, 5, 5]   # three minimal cuts: the largest foreground wins
    assert GC.solved("zero16")["labels"].all() and GC.solved("zero16")["flow"] == 0
    assert not GC.solved("allbg16")["labels"].any()
    assert GC.solved("wide64x32")["flow"] == 1 << 31       # beyond int32


def test_oracle_round_cap_and_topology_errors():
    N, coo, cs, ct, ce = GC.solver_case("grid16")
    capped = GO.solve(N, coo, cs, ct, ce, max_rounds=1)
    assert capped["converged"] == 0 and capped["rounds"] == 1
    for bad, msg in ((np.array([[0], [1]]), "reverse"), (np.array([[0, 1, 0], [1, 0, 1]]), "duplicate"), (np.array([[0, 1, 1], [1, 0, 1]]), "self")):
        with pytest.raises(ValueError, match=msg):
            GO.csr_by_source(bad, 2)


def test_oracle_capacities_quantisation():
    coo = GC.grid_edges(2, 2)
    cs, ct, ce = GO.capacities(np.array([0.0, 1.0, 0.5, 0.25], np.float32), coo, intensity=np.array([0, 0, 10, 255], np.float32))
    big = int(np.rint(-np.log(1e-6) * 1024))               # the clamp: p = 0 and p = 1 count as 1e-6 and 1 - 1e-6
    assert ct.tolist() == [big, 0, 710, 1420] and cs.tolist() == [0, big, 710, 295]
    assert np.array_equal(ce, ce[[list(zip(*coo)).index((b, a)) for a, b in zip(*coo)]])
    assert set(ce.tolist()) == {1024, int(np.rint(np.exp(-0.5) * 1024)), 0}
    assert GO.capacities(np.array([0.0, 1.0, 0.5, 0.25], np.float32), coo, unit=2.0 ** 17)[1][0] == 1 << 20   # the ceiling
    assert GO.quant(np.array([0.5 / 1024, 1.5 / 1024, 2.5 / 1024])).tolist() == [0, 2, 2]                      # ties to even, as lrintf
    assert np.array_equal(GO.prior_from_counts(np.array([[3, 1], [0, 0]]), 1), [2 / 6, 1 / 2])


def test_api_surface_without_a_device():
    import torch
    for name in ("graph_cut", "cut_capacities", "cut_energy", "GraphCut"):
        assert hasattr(mgunet, name) and name in mgunet.__all__
    from mgunet import graphcut  # noqa: F401
    assert callable(mgunet.MinCutRefinement.solve) and callable(mgunet.MinCutRefinement.refine_patches)
    m = mgunet.MinCutRefinement(0.25, 7.0, 2.0)
    assert (m.gamma_unet_priors, m.sigma_intensity, m.sigma_features) == (0.25, 7.0, 2.0)
    args = (None, None, None, m, None, None)
    with pytest.raises(ValueError, match="num_segments must be 2"):
        mgunet.MinGraphUNetE2E(*args, num_segments=3, partition="mincut")
    with pytest.raises(ValueError, match="partition must be"):
        mgunet.MinGraphUNetE2E(*args, num_segments=2, partition="graphcut")
    assert mgunet.MinGraphUNetE2E(*args, num_segments=3).partition == "predictor"
    assert mgunet.MinGraphUNetE2E(*args, num_segments=2, partition="mincut").partition == "mincut"
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # a CPU tensor is refused, not computed
        mgunet.graph_cut(ei, torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mgunet.cut_capacities(torch.full((2,), 0.5), ei)
    with pytest.raises(ValueError, match="int64"):
        mgunet.graph_cut(ei.to(torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
