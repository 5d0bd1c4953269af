"""The graph cut on the device (mgunet.graph_cut / cut_capacities / cut_energy, MinCutRefinement.solve / refine_patches,
MinGraphUNetE2E(partition="mincut")) against the numpy oracle of tests/graphcut_oracle.py, which the CPU tier checks against scipy.
Capacities are integers, the max-flow value and the minimal sink side of the cut are unique: labels, flow and converged are compared
bit for bit although the kernel uses atomics.  The shapes are the smallest that reach every path: fewer nodes than a wave, a node count
that is a multiple of no workgroup size (33 x 31), unsorted CSR rows, asymmetric capacities, an excess and a flow beyond 32 bits, and the
64 x 64 patch grid that fills the LDS budget (the only size at which the > 64 KiB opt-in is taken)."""
import functools

import numpy as np
import pytest
import torch

import graphcut_cases as GC
import graphcut_oracle as GO
import mgunet
import mgunet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
I32 = torch.int32


def dev_case(name):
    N, coo, cs, ct, ce = GC.solver_case(name)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)   # noqa: E731
    return N, t(coo, torch.int64), t(cs, I32), t(ct, I32), t(ce, I32)


def assert_cut_equals_oracle(cut, names):
    cut.check()
    for b, name in enumerate(names):
        ref = GC.solved(name)
        assert int(cut.converged[b]) == ref["converged"] == 1, name
        assert int(cut.flow[b]) == ref["flow"], (name, int(cut.flow[b]), ref["flow"])
        assert np.array_equal(cut.labels[b].cpu().numpy(), ref["labels"]), (name, int((cut.labels[b].cpu().numpy() != ref["labels"]).sum()))
        assert 0 <= int(cut.rounds[b]) <= (8 * len(ref["labels"]) + 64) // 10


@pytest.mark.parametrize("name", ["n1", "n2", "isolated", "tie", "grid5x7", "grid16", "grid33x31", "random200"])
def test_solver_equals_oracle(cuda, name):
    N, ei, cs, ct, ce = dev_case(name)
    before = [t.clone() for t in (cs, ct, ce)]
    cut = mgunet.graph_cut(ei, cs, ct, ce, num_nodes=N)
    assert cut.labels.dtype == torch.uint8 and tuple(cut.labels.shape) == (1, N) and cut.flow.dtype == torch.int64
    assert cut.rounds.dtype == I32 and cut.converged.dtype == I32
    assert_cut_equals_oracle(cut, [name])
    assert int(cut.rounds[0]) == GC.solved(name)["rounds"]        # the oracle runs the kernel's schedule
    assert all(torch.equal(a, b) for a, b in zip(before, (cs, ct, ce)))
    assert int(mgunet.cut_energy(cut.labels, ei, cs, ct, ce)[0]) == GC.solved(name)["flow"]
    if name == "tie":
        assert cut.labels.tolist() == [[1, 1]] and int(cut.flow[0]) == 5
    if name == "random200":                                         # the case has asymmetric capacities: the reverse index is exercised
        N_, coo, _, _, ce_np = GC.solver_case(name)
        pos = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(*coo))}
        assert any(ce_np[k] != ce_np[pos[(b, a)]] for (a, b), k in pos.items())
    for period, threads in ((1, 64), (5, 1024)):                    # the result does not depend on the tuning parameters
        other = mgunet.graph_cut(ei, cs, ct, ce, relabel_period=period, threads=threads)
        assert torch.equal(other.labels, cut.labels) and torch.equal(other.flow, cut.flow) and int(other.converged[0]) == 1


def test_batch_of_three_on_one_topology(cuda):
    """all capacities 0 (flow 0, every node foreground by the tie rule) | forced all-background by huge sink arcs | a mixed graph"""
    names = ["zero16", "allbg16", "grid16"]
    cases = [dev_case(n) for n in names]
    ei = cases[0][1]
    assert all(torch.equal(c[1], ei) for c in cases)
    cs, ct, ce = (torch.cat([c[i] for c in cases]) for i in (2, 3, 4))
    cut = mgunet.graph_cut(ei, cs, ct, ce, batch=3)
    assert_cut_equals_oracle(cut, names)
    assert int(cut.flow[0]) == 0 and bool(cut.labels[0].all()) and not bool(cut.labels[1].any())
    assert 0 < int(cut.labels[2].sum()) < 256
    assert torch.equal(mgunet.cut_energy(cut.labels, ei, cs, ct, ce, batch=3), cut.flow)


@pytest.mark.parametrize("name,total", [("wide32", 1 << 30), ("wide64x32", 1 << 31)])
def test_excess_and_flow_beyond_32_bits(cuda, name, total):
    N, ei, cs, ct, ce = dev_case(name)
    assert int(cs.to(torch.int64).sum()) == total
    cut = mgunet.graph_cut(ei, cs, ct, ce)
    assert_cut_equals_oracle(cut, [name])
    assert int(cut.flow[0]) == GC.solved(name)["flow"] == total     # every source arc is carried to the two sink nodes


def test_full_lds_budget_64x64(cuda):
    name = "full64"
    N, ei, cs, ct, ce = dev_case(name)
    assert (N, ei.shape[1]) == (4096, 16128)
    cut = mgunet.graph_cut(ei, cs, ct, ce)
    assert_cut_equals_oracle(cut, [name])
    flow = int(cut.flow[0])
    assert int(mgunet.cut_energy(cut.labels, ei, cs, ct, ce)[0]) == flow
    # no other labelling is cheaper: 64 single-node flips and 16 flips of a 3 x 3 block, one batched energy call
    rng = np.random.RandomState(5)
    lab = np.repeat(GC.solved(name)["labels"][None], 80, 0).reshape(80, 64, 64)
    for i in range(64):
        y, x = rng.randint(0, 64, 2)
        lab[i, y, x] ^= 1
    for i in range(64, 80):
        y, x = rng.randint(0, 62, 2)
        lab[i, y:y + 3, x:x + 3] ^= 1
    rep = lambda t: t.repeat(80)   # noqa: E731
    en = mgunet.cut_energy(torch.from_numpy(lab).to(DEV), ei, rep(cs), rep(ct), rep(ce), batch=80).cpu().numpy()
    assert (en >= flow).all(), (int(en.min()), flow)
    N_, coo, cs_np, ct_np, ce_np = GC.solver_case(name)
    assert [int(e) for e in en[[0, 40, 79]]] == [GO.energy(lab[i].ravel(), coo, cs_np, ct_np, ce_np) for i in (0, 40, 79)]


def test_two_solves_are_identical(cuda):
    N, ei, cs, ct, ce = dev_case("grid33x31")
    a, b = mgunet.graph_cut(ei, cs, ct, ce), mgunet.graph_cut(ei, cs, ct, ce)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.flow, b.flow) and torch.equal(a.rounds, b.rounds)
    assert torch.equal(a.converged, b.converged)


def test_round_cap_is_reported(cuda):
    N, ei, cs, ct, ce = dev_case("grid16")
    before = [t.clone() for t in (cs, ct, ce)]
    cut = mgunet.graph_cut(ei, cs, ct, ce, max_rounds=1)
    assert int(cut.converged[0]) == 0 and int(cut.rounds[0]) == 1
    with pytest.raises(RuntimeError, match="did not converge"):
        cut.check()
    assert all(torch.equal(a, b) for a, b in zip(before, (cs, ct, ce)))


def test_refusals(cuda, monkeypatch):
    from mgunet import _lib
    launched = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (launched.append(name), real(name, *a, **k))[1])
    z = lambda n: torch.zeros(n, dtype=I32, device=DEV)   # noqa: E731
    for edges, msg in (([[0, 1, 1], [1, 0, 2]], "without its reverse"), ([[0, 1, 0, 1], [1, 0, 1, 0]], "duplicate"),
                       ([[0, 1, 2], [1, 0, 2]], "self loop")):
        ei = torch.tensor(edges, dtype=torch.int64, device=DEV)
        with pytest.raises(ValueError, match=msg):
            mgunet.graph_cut(ei, z(3), z(3), z(ei.shape[1]))
    with pytest.raises(IndexError):
        mgunet.graph_cut(torch.tensor([[0, 3], [3, 0]], device=DEV), z(3), z(3), z(2))
    ei = torch.from_numpy(GC.grid_edges(96, 96)).to(DEV)             # 20 N + 4 E + 40 = 330 KB: over any workgroup's LDS
    with pytest.raises(ValueError, match=r"bytes of LDS.*workgroup \d+"):
        mgunet.graph_cut(ei, z(96 * 96), z(96 * 96), z(ei.shape[1]))
    with pytest.raises(ValueError, match="num_segments must be 2"):
        mgunet.MinGraphUNetE2E(None, None, None, mgunet.MinCutRefinement(), None, None, num_segments=3, partition="mincut")
    with pytest.raises(ValueError, match="cap_edge"):
        mgunet.graph_cut(torch.tensor([[0, 1], [1, 0]], device=DEV), z(2), z(2), z(3))
    torch.cuda.synchronize()
    assert launched.count("mgu_graphcut_solve") == 1                 # only the over-budget call got as far as the entry point, which refused it


# ---- capacities ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cap_inputs(D):
    rng = np.random.RandomState(40 + D)
    H, W, B = 6, 5, 2
    N = H * W
    coo = GC.grid_edges(H, W, 2)
    prior = rng.rand(B * N).astype(np.float32)
    prior[[0, 1, 2, 3]] = [0.0, 1.0, 1e-7, 1.0 - 2.0 ** -24]         # the clamp on both sides
    counts = rng.randint(0, 257, (B * N, 3)).astype(np.int32)
    counts[0], counts[1], counts[2] = (0, 0, 0), (0, 256, 0), (256, 0, 0)
    inten = (rng.rand(B * N) * 255).astype(np.float32)
    inten[N:] = np.round(inten[N:] / 8) * 2                          # image 1: close intensities, weights near 1
    feats = (rng.randn(B * N, D) * rng.uniform(0.05, 1.0, (B * N, 1)) / np.sqrt(D)).astype(np.float32)   # near and far neighbours
    return H, W, B, N, coo, prior, counts, inten, feats


@pytest.mark.parametrize("kind", ["prob", "counts"])
@pytest.mark.parametrize("combo", ["prior", "intensity", "features", "both"])
@pytest.mark.parametrize("D", [8, 12, 64])
def test_capacities_against_float64(cuda, D, combo, kind):
    H, W, B, N, coo, prior, counts, inten, feats = cap_inputs(D)
    use_i, use_f = combo in ("intensity", "both"), combo in ("features", "both")
    kw = dict(gamma=0.7, sigma_intensity=9.0, sigma_features=0.8, smoothness=1.5)
    ei = torch.from_numpy(coo).to(DEV)
    td = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    pr = td(prior) if kind == "prob" else td(counts)
    cs, ct, ce = mgunet.cut_capacities(pr, ei, td(inten) if use_i else None, td(feats) if use_f else None,
                                       counts_foreground=1 if kind == "counts" else None, batch=B, **kw)
    assert cs.dtype == ct.dtype == ce.dtype == I32 and cs.shape == ct.shape == (B * N,) and ce.shape == (B * coo.shape[1],)
    p64 = prior.astype(np.float64) if kind == "prob" else GO.prior_from_counts(counts, 1)
    E = coo.shape[1]
    pos = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(*coo))}
    rev = np.array([pos[(int(b), int(a))] for a, b in zip(*coo)])
    worst = 0
    for b in range(B):
        s = slice(b * N, (b + 1) * N)
        rs, rt, re = GO.capacities(p64[s], coo, inten[s] if use_i else None, feats[s] if use_f else None, **kw)
        got = [x.cpu().numpy().astype(np.int64) for x in (cs[s], ct[s], ce[b * E:(b + 1) * E])]
        worst = max([worst] + [int(np.abs(g - r).max()) for g, r in zip(got, (rs, rt, re))])
        assert np.array_equal(got[2], got[2][rev])                   # bitwise symmetric
        assert bool(got[2].any()) == (use_i or use_f)                # neither input: the edges carry no weight
    print(f"capacities D={D} {combo} {kind}: max |gpu - float64| = {worst} unit(s)")
    assert worst <= 1
    assert not (use_i or use_f) or (int(ce.max()) > 512 and len(torch.unique(ce)) > 20)   # the comparison is not one of zeros
    big = int(np.rint(-np.log(1e-6) * 1024))                         # the documented clamp: 14147 against 0
    if kind == "prob":
        assert (int(ct[0]), int(cs[0]), int(ct[1]), int(cs[1])) == (big, 0, 0, big)
        assert (int(ct[2]), int(cs[3])) == (big, big)
    else:
        assert int(ct[0]) == int(cs[0]) == 710                       # no pixel counted: p = 1/2
        assert int(ct[1]) == int(np.rint(-np.log(257 / 258) * 1024)) and int(cs[1]) == int(np.rint(-np.log(1 / 258) * 1024))


def test_capacity_ceiling_and_unit(cuda):
    H, W, B, N, coo, prior, counts, inten, feats = cap_inputs(8)
    ei = torch.from_numpy(coo).to(DEV)
    cs, ct, ce = mgunet.cut_capacities(torch.from_numpy(prior).to(DEV), ei, torch.from_numpy(inten).to(DEV), batch=B, unit=2 ** 17, smoothness=16.0)
    assert int(ct[0]) == int(cs[1]) == 1 << 20 and int(ct.max()) == int(cs.max()) == int(ce.max()) == 1 << 20
    rs, rt, re = GO.capacities(prior[:N].astype(np.float64), coo, inten[:N], unit=2.0 ** 17, smoothness=16.0)
    assert np.abs(ct[:N].cpu().numpy() - rt).max() <= 1 and np.abs(ce[:coo.shape[1]].cpu().numpy() - re).max() <= 1   # 2^20 * 2^-22 < 1


# ---- wiring -------------------------------------------------------------------------------------------------------------------------
def tiny_e2e(partition):
    cfg = (3, 2, 8, 3)
    torch.manual_seed(3)
    unet = mgunet.UNet(*cfg); unet.load_state_dict(O.make_unet_params(*cfg, seed=11))
    pgat = mgunet.GATNetwork(8, 16, 8, 2); pgat.load_state_dict(O.make_gat_params(8, 16, 8, 2, 1, seed=2))
    rgat = mgunet.GATNetwork(8, 16, 8, 2); rgat.load_state_dict(O.make_gat_params(8, 16, 8, 2, 1, seed=4))
    pred = mgunet.PatchSegmentPredictor(8, 2)
    det = mgunet.DetectionHead(16, 1)
    kw = {} if partition is None else {"partition": partition}
    return mgunet.MinGraphUNetE2E(unet, pgat, pred, mgunet.MinCutRefinement(0.6, 12.0, 0.7), rgat, det, num_segments=2, **kw).to(DEV).eval()


def test_e2e_mincut_partition_is_the_hand_composition(cuda):
    B, H, W, p = 2, 64, 48, 16
    x = torch.from_numpy(O.formula_normal("tiny/c/x", (B, 3, H, W), seed=11)).to(DEV)
    u8 = torch.from_numpy(np.random.RandomState(9).randint(0, 256, (B, H, W, 3)).astype(np.uint8)).to(DEV)
    model = tiny_e2e("mincut")
    with pytest.raises(ValueError, match="images_u8"):
        model(x)
    out = model(x, images_u8=u8)
    # by hand, on the same logits, bytes and embeddings
    emb, mc = out["node_embeddings"], model.mincut
    _, counts = mgunet.patch_labels(out["logits"], p, return_counts=True)
    inten = torch.cat([mgunet.patch_features_u8(img, p) for img in u8]).reshape(-1)
    ei = model.core.graph.edge_index(H, W, x.device)
    cs, ct, ce = mgunet.cut_capacities(counts, ei, inten, emb, counts_foreground=1, gamma=mc.gamma_unet_priors, sigma_intensity=mc.sigma_intensity,
                                       sigma_features=mc.sigma_features, batch=B)
    cut = mgunet.graph_cut(ei, cs, ct, ce, batch=B).check()
    want = cut.labels.reshape(-1).to(torch.int64)
    assert out["cut_labels"].dtype == torch.int64 and torch.equal(out["cut_labels"], want) and torch.equal(out["hard_labels"], want)
    assert torch.equal(out["cut_energy"], cut.flow.to(torch.float64) / 1024)
    N = (H // p) * (W // p)
    for b in range(B):                                               # and the labels are the oracle's cut of those capacities
        s, e = slice(b * N, (b + 1) * N), slice(b * ei.shape[1], (b + 1) * ei.shape[1])
        ref = GO.solve(N, ei.cpu().numpy(), cs[s].cpu().numpy(), ct[s].cpu().numpy(), ce[e].cpu().numpy())
        assert np.array_equal(cut.labels[b].cpu().numpy(), ref["labels"]) and int(cut.flow[b]) == ref["flow"]
    region, fused = mgunet.region_stage(emb, want, B, 2, model.region_gat, H // p, W // p, H, W, f_u=out["decoder_feats"][0])
    assert torch.equal(out["region_embeddings"], region) and torch.equal(out["fused"], fused)

    # the default partition: today's keys and today's values
    base = tiny_e2e(None)
    ref = base(x)
    assert base.partition == "predictor"
    assert set(ref) == {"logits", "skips", "decoder_feats", "node_embeddings", "loss_partition", "soft_assignments", "hard_labels",
                        "region_embeddings", "fused", "bboxes", "confidence"}
    lg, _, ft, e2 = base.core(x)
    losses, soft, hard = base.mincut.forward_batched(e2, ei, B, 2, base.segment_predictor(e2).contiguous())
    r2, f2 = mgunet.region_stage(e2, hard, B, 2, base.region_gat, H // p, W // p, H, W, f_u=ft[0])
    det = base.detection_head(f2)
    assert torch.equal(ref["logits"], lg) and torch.equal(ref["hard_labels"], hard) and torch.equal(ref["soft_assignments"], soft)
    assert torch.equal(ref["loss_partition"], losses.mean()) and torch.equal(ref["region_embeddings"], r2) and torch.equal(ref["fused"], f2)
    assert torch.equal(ref["bboxes"], det[0]) and torch.equal(ref["confidence"], det[1])
    assert torch.equal(ref["hard_labels"], hard) and torch.equal(base(x, images_u8=u8)["hard_labels"], hard)   # the bytes are ignored
    # same weights (same seeds): what the predictor produced is untouched by the cut
    assert torch.equal(out["soft_assignments"], ref["soft_assignments"]) and torch.equal(out["loss_partition"], ref["loss_partition"])
