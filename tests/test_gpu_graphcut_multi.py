"""The K-label graph cut on the device (mgunet.label_costs / graph_cut_multi / cut_energy_multi, MinCutRefinement.solve_multi /
refine_patches_multi, MinGraphUNetE2E(partition="expansion")) against the numpy oracle of tests/graphcut_multi_oracle.py, which the CPU
tier checks against scipy and brute force.  Everything is an integer problem with a canonical answer per move: labels, energy, moves,
accepted, rounds and converged are compared bit for bit.  The shapes are the smallest that reach every path: one node, one label, a
node count that is a multiple of no workgroup size (33 x 31), several nodes per thread (64 x 32), unsorted CSR rows (random200) and the
64 x 64 grid that fills the LDS budget."""
import numpy as np
import pytest
import torch

import graphcut_cases as GC
import graphcut_multi_cases as MC
import graphcut_multi_oracle as GMO
import mgunet
import mgunet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I32 = torch.int32
FIELDS = ("energy", "moves", "accepted", "rounds", "converged")


def td(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)


def dev_case(name):
    N, coo, U, ce, init = MC.multi_case(name)
    return N, td(coo, torch.int64), td(U, I32), td(ce, I32), None if init is None else td(init, torch.uint8).reshape(1, N)


def assert_equals_oracle(cut, refs):
    for b, ref in enumerate(refs):
        got = {f: int(getattr(cut, f)[b]) for f in FIELDS}
        assert got == {f: ref[f] for f in FIELDS}, (b, got, {f: ref[f] for f in FIELDS})
        lab = cut.labels[b].cpu().numpy()
        assert np.array_equal(lab, ref["labels"]), (b, int((lab != ref["labels"]).sum()))


@pytest.mark.parametrize("name", MC.MULTI_CASES)
def test_expansion_equals_oracle(cuda, name):
    N, ei, U, ce, init = dev_case(name)
    before = [t.clone() for t in (ei, U, ce)] + ([init.clone()] if init is not None else [])
    cut = mgunet.graph_cut_multi(ei, U, ce, init=init)
    assert cut.labels.dtype == torch.uint8 and tuple(cut.labels.shape) == (1, N) and cut.energy.dtype == torch.int64
    assert all(getattr(cut, f).dtype == I32 and tuple(getattr(cut, f).shape) == (1,) for f in FIELDS[1:])
    cut.check()
    assert_equals_oracle(cut, [MC.expanded(name)])
    assert torch.equal(mgunet.cut_energy_multi(cut.labels, ei, U, ce), cut.energy)
    assert all(torch.equal(a, b) for a, b in zip(before, [ei, U, ce] + ([init] if init is not None else [])))   # inputs untouched
    if name == "tiepair":
        assert cut.labels.tolist() == [[0, 1]] and int(cut.accepted[0]) == 0          # both moves tie and are dropped
    if name == "zero16":
        assert not bool(cut.labels.any()) and int(cut.moves[0]) == 3
    if name == "full64":
        assert (N, ei.shape[1]) == (4096, 16128)
    if name == "random200":
        assert int(torch.bincount(ei[0]).max()) == 9


def test_batch_of_three_different_graphs(cuda):
    names = ["zero16", "grid16b", "init16"]                                           # K = 3 | 3 | 4 columns: pad to one K = 4 problem
    cases = [MC.multi_case(n) for n in names]
    coo = cases[0][1]
    assert all(np.array_equal(c[1], coo) for c in cases)
    N, K = 256, 4
    Us = [np.concatenate([c[2], np.full((N, K - c[2].shape[1]), 1 << 20)], 1) for c in cases]   # a label nobody can afford
    inits = [np.full(N, 255) if c[4] is None else c[4] for c in cases]                # 255: the node's cheapest label
    refs = [GMO.expand(N, coo, u, c[3], init=i) for u, c, i in zip(Us, cases, inits)]
    ei = td(coo, torch.int64)
    U, ce, init = td(np.concatenate(Us), I32), td(np.concatenate([c[3] for c in cases]), I32), td(np.stack(inits), torch.uint8)
    cut = mgunet.graph_cut_multi(ei, U, ce, batch=3, init=init).check()
    assert_equals_oracle(cut, refs)
    assert len({r["energy"] for r in refs}) == 3 and refs[1]["accepted"] > 0 and refs[2]["accepted"] > 0
    assert torch.equal(mgunet.cut_energy_multi(cut.labels, ei, U, ce, batch=3), cut.energy)
    assert torch.equal(mgunet.graph_cut_multi(ei, U.reshape(3, N, K), ce, batch=3, init=init).labels, cut.labels)   # (B, N, K) costs


def test_two_labels_from_zero_are_graph_cut_itself(cuda):
    N, ei, U, ce, init = dev_case("binary16")
    multi = mgunet.graph_cut_multi(ei, U, ce, init=init).check()
    binary = mgunet.graph_cut(ei, U[:, 0].contiguous(), U[:, 1].contiguous(), ce).check()
    assert torch.equal(multi.labels, binary.labels) and torch.equal(multi.energy, binary.flow)
    assert_equals_oracle(multi, [MC.expanded("binary16")])
    assert torch.equal(mgunet.cut_energy_multi(binary.labels, ei, U, ce), binary.flow)


def test_cycle_cap_is_reported_and_leaves_a_labelling(cuda):
    N, ei, U, ce, _ = dev_case("grid33x31")
    _, coo, U_np, ce_np, _ = MC.multi_case("grid33x31")
    cut = mgunet.graph_cut_multi(ei, U, ce, max_cycles=1)
    assert_equals_oracle(cut, [GMO.expand(N, coo, U_np, ce_np, max_cycles=1)])
    assert int(cut.converged[0]) == 0 and int(cut.moves[0]) == 5
    with pytest.raises(RuntimeError, match="did not converge"):
        cut.check()
    assert int(cut.labels.max()) < 5
    start = torch.from_numpy(GMO.start_labels(U_np)).to(DEV)
    e_start = mgunet.cut_energy_multi(start, ei, U, ce)
    assert torch.equal(mgunet.cut_energy_multi(cut.labels, ei, U, ce), cut.energy) and int(cut.energy[0]) <= int(e_start[0])
    assert int(e_start[0]) == GMO.energy_multi(GMO.start_labels(U_np), coo, U_np, ce_np)
    capped = mgunet.graph_cut_multi(ei, U, ce, max_rounds=1)                          # the first move's solve hits the round cap
    assert_equals_oracle(capped, [GMO.expand(N, coo, U_np, ce_np, max_rounds=1)])
    assert int(capped.converged[0]) == 0 and torch.equal(capped.labels[0], start.to(torch.uint8))


def test_reproducible_and_independent_of_the_tuning_parameters(cuda):
    N, ei, U, ce, _ = dev_case("grid33x31")
    a, b = mgunet.graph_cut_multi(ei, U, ce), mgunet.graph_cut_multi(ei, U, ce)
    assert all(torch.equal(getattr(a, f), getattr(b, f)) for f in FIELDS + ("labels",))
    for period, threads in ((1, 64), (5, 1024), (1000, 256)):
        o = mgunet.graph_cut_multi(ei, U, ce, relabel_period=period, threads=threads)
        assert all(torch.equal(getattr(a, f), getattr(o, f)) for f in ("labels", "energy", "moves", "accepted", "converged")), (period, threads)
    _, coo, U_np, ce_np, _ = MC.multi_case("grid33x31")
    o = mgunet.graph_cut_multi(ei, U, ce, relabel_period=5, threads=128)
    assert int(o.rounds[0]) == GMO.expand(N, coo, U_np, ce_np, period=5)["rounds"]    # rounds follow the period, not the workgroup size


def test_label_costs_against_float64(cuda):
    rng = np.random.RandomState(50)
    counts = rng.randint(0, 257, (2, 30, 5)).astype(np.int32)
    counts[0, 0], counts[0, 1], counts[0, 2] = 0, (0, 256, 0, 0, 0), (256, 0, 0, 0, 0)
    got = mgunet.label_costs(td(counts, I32), batch=2)
    assert got.dtype == I32 and tuple(got.shape) == (60, 5)
    assert np.array_equal(got.cpu().numpy(), GMO.label_costs(counts.reshape(60, 5)))   # exact
    assert torch.equal(mgunet.label_costs(td(counts.reshape(60, 5), I32)), got)
    assert got[0].tolist() == [int(np.rint(-np.log(1 / 5) * 1024))] * 5                # no pixel counted: p = 1 / K
    prob = MC.class_maps(12, 10, 5, 33)[0]                                            # the inputs the CPU tier checks the condition on
    prob[0, :4] = [0.0, 1.0, 1e-7, 1.0 - 2.0 ** -24]
    out = mgunet.label_costs(td(prob, torch.float32)).cpu().numpy().astype(np.int64)
    d = np.abs(out - GMO.label_costs(prob))
    print(f"label_costs probabilities: max |gpu - float64| = {int(d.max())} unit(s), share differing = {float((d != 0).mean()):.5f}")
    assert d.max() <= 1 and (d != 0).mean() <= 1e-3
    big = int(np.rint(-np.log(1e-6) * 1024))
    assert out[0, :4].tolist() == [big, 0, big, 0]
    assert int(mgunet.label_costs(td(prob, torch.float32), unit=2 ** 17)[0, 0]) == 1 << 20   # the ceiling
    two = rng.randint(0, 257, (40, 2)).astype(np.int32)                               # K = 2: the binary prior (n_fg + 1) / (n_all + 2)
    assert np.array_equal(mgunet.label_costs(td(two, I32)).cpu().numpy(), GMO.label_costs(two))


def tiny_e2e(num_segments, classes=3):
    cfg = (3, classes, 8, 3)
    torch.manual_seed(3)
    unet = mgunet.UNet(*cfg); unet.load_state_dict(O.make_unet_params(*cfg, seed=11))
    pgat = mgunet.GATNetwork(8, 16, 8, 2); pgat.load_state_dict(O.make_gat_params(8, 16, 8, 2, 1, seed=2))
    rgat = mgunet.GATNetwork(8, 16, 8, 2); rgat.load_state_dict(O.make_gat_params(8, 16, 8, 2, 1, seed=4))
    pred = mgunet.PatchSegmentPredictor(8, num_segments)
    det = mgunet.DetectionHead(16, 1)
    return mgunet.MinGraphUNetE2E(unet, pgat, pred, mgunet.MinCutRefinement(0.6, 12.0, 0.7), rgat, det, num_segments=num_segments,
                                  partition="expansion").to(DEV).eval()


def test_refine_patches_multi_is_the_hand_composition(cuda):
    B, C, H, W, p = 2, 3, 64, 64, 16
    rng = np.random.RandomState(61)
    logits = torch.from_numpy(rng.randn(B, C, H, W).astype(np.float32) + 2.0 * MC.class_maps(H, W, C, 62)[0].T.reshape(1, C, H, W)).to(DEV)
    u8 = torch.from_numpy(rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(DEV)
    feats = torch.from_numpy(rng.randn(B * 16, 8).astype(np.float32) * 0.5).to(DEV)
    mc = mgunet.MinCutRefinement(0.6, 12.0, 0.7)
    hard, energy, cut = mc.refine_patches_multi(logits, u8, feats, p)
    cut.check()
    _, counts = mgunet.patch_labels(logits, p, return_counts=True)
    U = mgunet.label_costs(counts, batch=B)
    inten = torch.cat([mgunet.patch_features_u8(img, p) for img in u8]).reshape(-1)
    ei = mgunet.PatchGraphConstructor(p).edge_index(H, W, torch.device(DEV))
    ce = mgunet.cut_capacities(torch.full((B * 16,), 0.5, device=DEV), ei, inten, feats, gamma=0.6, sigma_intensity=12.0, sigma_features=0.7, batch=B)[2]
    want = mgunet.graph_cut_multi(ei, U, ce, batch=B).check()
    assert hard.dtype == torch.int64 and torch.equal(hard, want.labels.reshape(-1).to(torch.int64))
    assert energy.dtype == torch.float64 and torch.equal(energy, want.energy.to(torch.float64) / 1024)
    assert 0 <= int(hard.min()) and int(hard.max()) < C
    E = ei.shape[1]
    refs = [GMO.expand(16, ei.cpu().numpy(), U[b * 16:(b + 1) * 16].cpu().numpy(), ce[b * E:(b + 1) * E].cpu().numpy()) for b in range(B)]
    assert_equals_oracle(cut, refs)                                                   # and the labels are the oracle's for those inputs
    h2, e2, _ = mc.solve_multi(counts, ei, inten, feats, batch=B)
    assert torch.equal(h2, hard) and torch.equal(e2, energy)


def test_e2e_expansion_partition(cuda):
    B, H, W, p = 2, 64, 48, 16
    x = torch.from_numpy(O.formula_normal("tiny/c/x", (B, 3, H, W), seed=11)).to(DEV)
    u8 = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(DEV)
    model = tiny_e2e(3)
    with pytest.raises(ValueError, match="images_u8"):
        model(x)
    out = model(x, images_u8=u8)
    hard, energy, cut = model.mincut.refine_patches_multi(out["logits"], u8, out["node_embeddings"], p)
    cut.check()
    assert out["cut_labels"].dtype == torch.int64 and torch.equal(out["cut_labels"], hard) and torch.equal(out["hard_labels"], hard)
    assert 0 <= int(hard.min()) and int(hard.max()) < 3 and torch.equal(out["cut_energy"], energy)
    region, fused = mgunet.region_stage(out["node_embeddings"], hard, B, 3, model.region_gat, H // p, W // p, H, W, f_u=out["decoder_feats"][0])
    assert torch.equal(out["region_embeddings"], region) and torch.equal(out["fused"], fused)
    with pytest.raises(ValueError, match=r"3 classes.*num_segments is 4"):
        tiny_e2e(4)(x, images_u8=u8)


def test_refusals_before_any_launch(cuda, monkeypatch):
    from mgunet import _lib
    launched = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (launched.append(name), real(name, *a, **k))[1])
    z = lambda *s: torch.zeros(s, dtype=I32, device=DEV)   # noqa: E731
    ei = torch.from_numpy(GC.grid_edges(96, 96)).to(DEV)                              # 21 N + 4 E + 48 = 335 KB: over any workgroup's LDS
    with pytest.raises(ValueError, match=r"\d+ bytes of LDS.*workgroup \d+"):
        mgunet.graph_cut_multi(ei, z(96 * 96, 3), z(ei.shape[1]))
    pair = torch.tensor([[0, 1], [1, 0]], device=DEV)
    for K in (0, 256):
        with pytest.raises(ValueError, match="1 <= K <= 255"):
            mgunet.graph_cut_multi(pair, z(2, K), z(2))
        with pytest.raises(ValueError, match="1 <= K <= 255"):
            mgunet.label_costs(z(2, K))
        with pytest.raises(ValueError, match="1 <= K <= 255"):
            mgunet.cut_energy_multi(torch.zeros(2, dtype=torch.uint8, device=DEV), pair, z(2, K), z(2))
    with pytest.raises(TypeError, match="int32"):
        mgunet.graph_cut_multi(pair, torch.zeros((2, 3), device=DEV), z(2))
    with pytest.raises(TypeError, match="uint8"):
        mgunet.graph_cut_multi(pair, z(2, 3), z(2), init=torch.zeros((1, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="cap_edge"):
        mgunet.graph_cut_multi(pair, z(2, 3), torch.zeros(2, device=DEV))
    with pytest.raises(ValueError, match="int64"):
        mgunet.graph_cut_multi(pair.to(I32), z(2, 3), z(2))
    with pytest.raises(TypeError, match="float32 probabilities or int32"):
        mgunet.label_costs(torch.zeros((2, 3), dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError, match="integer"):
        mgunet.cut_energy_multi(torch.zeros(2, device=DEV), pair, z(2, 3), z(2))
    with pytest.raises(ValueError, match="do not split"):
        mgunet.graph_cut_multi(pair, z(3, 3), z(2), batch=2)
    # a star whose hub has degree 4095: a move's sink word could overflow, so the K-label path refuses it; the binary cut takes it
    N = 4096
    leaves = np.arange(1, N)
    star = torch.from_numpy(np.stack([np.concatenate([np.zeros(N - 1, np.int64), leaves]), np.concatenate([leaves, np.zeros(N - 1, np.int64)])])).to(DEV)
    for _ in range(2):                                                                # the second time from the topology cache
        with pytest.raises(ValueError, match="degree >= 4095"):
            mgunet.graph_cut_multi(star, z(N, 3), z(star.shape[1]))
    assert "mgu_graphcut_expand" in launched and launched.count("mgu_graphcut_expand") == 1   # only the over-budget call reached the entry point
    assert "mgu_graphcut_label_costs" not in launched and "mgu_graphcut_energy_multi" not in launched
    cs = torch.full((N,), 5, dtype=I32, device=DEV)
    cut = mgunet.graph_cut(star, cs, z(N), z(star.shape[1])).check()
    assert int(cut.flow[0]) == 0 and bool(cut.labels.all())
    sub = star[:, (star[0] < N - 1) & (star[1] < N - 1)].contiguous()                 # degree 4094 is taken
    ok = mgunet.graph_cut_multi(sub, z(N - 1, 3), z(sub.shape[1])).check()
    assert int(ok.energy[0]) == 0 and not bool(ok.labels.any())
