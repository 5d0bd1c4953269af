"""Deterministic cases, float64 references and the error bar of the graph attention kernels (csrc/gat.hip, gat_fused.hip, gat_bwd.hip)
at hubs, wide layers and max ties.  Plain torch / numpy on the CPU, everything drawn from the oracle's formula tensors: no fixture,
no GPU.  Imported by tests/test_gat_cases_host.py (case properties and the dev32 / devfx table, no GPU) and
tests/test_gpu_gat_f64.py (the kernels against the same references).

The reference is O.gat_head_forward per head and per graph (the max of graph_attention.py:86 is per graph) under torch autograd,
heads combined by cat or mean, train mode with explicit masks; a batch is ONE autograd graph, loss = sum_g (out_g * R_g).sum(), so
parameter gradients sum over graphs the way the kernels sum them.

The bar is the graph-branch rule (tests/graph_branch_cases.py) with one more term:

    err   = max|got - ref64| / max|ref64|          (no floor of 1; where ref64 is identically zero the result must be exactly zero)
    dev32 = the same measure of the oracle run in fp32 against the oracle run in float64
    devfx = the same measure of the fp32 oracle with torch.exp(v) replaced by torch.exp2((v * float32(log2 e)).float()): an fp32
            model of __expf, which every GAT kernel uses (its argument rounding costs about |v| * 6e-8 relative)
    bar   = max(4 * dev32, 4 * devfx, 16 * eps32)          (bar_of of graph_branch_cases.py with the devfx term)

Both deviations come from the oracle on the CPU, never from a kernel's output."""
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import torch

import mgunet_oracle as O
from graph_branch_cases import Ref, bar_of, general_graph, rel_err

ALPHA, P_DROP = 0.2, 0.3
LOG2E32 = torch.tensor(np.float32(np.log2(np.e)))


# ---- the oracle with one torch function swapped -----------------------------------------------------------------------------------
def exp_fx(v):
    """fp32 model of __expf: exp2 of the argument scaled by float32(log2 e), the product rounded to fp32."""
    return torch.exp2((v * LOG2E32.to(v.dtype)).float()).to(v.dtype)


@contextmanager
def oracle_with(exp=None, detach_max=False):
    """Runs O.gat_head_forward's own lines with torch.exp replaced (`exp`) and / or the graph-wide max of :86 cut out of the autograd
    graph (`detach_max`): the oracle stays the only statement of the formulas."""
    old_exp, old_max = torch.exp, torch.max
    try:
        if exp is not None:
            torch.exp = exp
        if detach_max:
            torch.max = lambda *a, **k: old_max(*a, **k).detach()
        yield
    finally:
        torch.exp, torch.max = old_exp, old_max


class GatRef(Ref):
    """Ref with the devfx term: bar = max(4 * dev32, 4 * devfx, 16 * eps32)."""

    def __init__(self, r64: dict, r32: dict, rfx: dict):
        super().__init__(r64, r32)
        self.devfx = {k: rel_err(rfx[k], self.r64[k]) for k in r64}

    def bar(self, name: str) -> float:
        return max(bar_of(self.dev32[name]), 4.0 * self.devfx[name])

    def check(self, name: str, got, log=None, what="") -> float:
        err, bar = rel_err(got, self.r64[name]), self.bar(name)
        if log is not None:
            log.append((what, name, self.dev32[name], self.devfx[name], bar, err))
        print(f"  {what:44s} {name:4s} dev32 {self.dev32[name]:.1e}  devfx {self.devfx[name]:.1e}  bar {bar:.1e}  err {err:.1e}")
        assert err <= bar, (what, name, "err", err, "bar", bar, "dev32", self.dev32[name], "devfx", self.devfx[name])
        return err


# ---- graphs: (2, E) int64 COO lists in arbitrary order ------------------------------------------------------------------------------
# in-degrees of ladder nodes 0..15: every boundary of the 4-slot, 8-slot and 64-id batches of gat_aggregate_kernel and of TRIP = 4 / 8
# of gat_fused2_kernel (129 = 33 / 17 trips).  Node LADDER_LONE has 64 in-edges between three edgeless rows on either side: the 4-row
# segment around it holds exactly 64 edges wherever the graph starts in a batch; the segments of nodes 11..14 hold more.
LADDER_DEG = (0, 1, 3, 4, 5, 7, 8, 9, 12, 16, 17, 63, 64, 65, 129, 2)
LADDER_N, LADDER_LONE = 40, 27
GEN_SEED = 21
SPUR_N, SPUR_HUB = 41, 9
PLATEAU_A, PLATEAU_N = 12, 32


def _shuffled(src, tgt, name):
    order = np.argsort(O.formula_uniform(name + "/order", (len(src),), 0.0, 1.0, 1), kind="stable")
    return torch.from_numpy(np.ascontiguousarray(np.stack([src, tgt])[:, order].astype(np.int64)))


def _rows(deg, name):
    deg = np.asarray(deg, dtype=np.int64)
    tgt = np.repeat(np.arange(len(deg)), deg)
    u = O.formula_uniform(name + "/src", (len(tgt),), 0.0, 1.0, 2).astype(np.float64)
    return _shuffled(np.minimum((u * len(deg)).astype(np.int64), len(deg) - 1), tgt, name)


def ladder_degrees():
    deg = np.zeros(LADDER_N, dtype=np.int64)
    deg[:len(LADDER_DEG)] = LADDER_DEG
    deg[LADDER_LONE] = 64
    return deg


def ladder_graph():
    return _rows(ladder_degrees(), "gat64/ladder")


def spur_graph():
    """41 nodes, node 9 with 70 in-edges between rows of 2 and 5, rows 20..39 with one each: E = 97."""
    deg = np.zeros(SPUR_N, dtype=np.int64)
    deg[SPUR_HUB], deg[SPUR_HUB - 1], deg[SPUR_HUB + 1], deg[20:40] = 70, 2, 5, 1
    return _rows(deg, "gat64/spur")


def grid_graph():
    return torch.from_numpy(np.ascontiguousarray(O.patch_graph_edges(80, 112, 16)))   # 5 x 7 patches, 116 edges


def tiny_graph():
    return torch.zeros((2, 1), dtype=torch.int64)


def edgeless():
    return torch.zeros((2, 0), dtype=torch.int64)


def plateau_graph():
    """Group A = nodes 0..11, group B = nodes 12..31; edges only A -> A (40) and B -> B (80)."""
    ua = O.formula_uniform("gat64/plateau/a", (2, 40), 0.0, 1.0, 3).astype(np.float64)
    ub = O.formula_uniform("gat64/plateau/b", (2, 80), 0.0, 1.0, 4).astype(np.float64)
    a, b = np.minimum((ua * PLATEAU_A).astype(np.int64), PLATEAU_A - 1), PLATEAU_A + np.minimum((ub * 20).astype(np.int64), 19)
    return _shuffled(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), "gat64/plateau")



@lru_cache(maxsize=None)
def batch(name):
    """[(edge_index with local ids, nodes)] of a batch; the graphs sit behind one another in node and in edge order."""
    gen = lambda N, E, seed: (general_graph(N, E, seed), N)
    if name == "dense":
        return [gen(101, 600, GEN_SEED), (edgeless(), 5), (ladder_graph(), LADDER_N), (tiny_graph(), 1)]
    if name == "big":
        return [gen(600, 3000, GEN_SEED + 1), (edgeless(), 5), (ladder_graph(), LADDER_N), (tiny_graph(), 1)]
    if name == "sparse":
        return [(grid_graph(), 35), (grid_graph(), 35), (spur_graph(), SPUR_N)]
    if name == "many":        # 14 graphs: G * heads > 256 at 32 heads
        return [(tiny_graph(), 1)] * 13 + [(ladder_graph(), LADDER_N)]
    if name == "general":
        return [gen(101, 600, GEN_SEED)]
    if name == "plateau":
        return [(plateau_graph(), PLATEAU_N)]
    raise KeyError(name)


@lru_cache(maxsize=None)
def layout(name):
    """(edge_index (2, E) with batch-wide ids, graph_ptr list, [(local edge_index, node lo, node hi, edge lo, edge hi)])."""
    parts, eis, gp, e0 = [], [], [0], 0
    for ei, n in batch(name):
        lo = gp[-1]
        parts.append((ei, lo, lo + n, e0, e0 + ei.shape[1]))
        eis.append(ei + lo)
        gp.append(lo + n)
        e0 += ei.shape[1]
    return torch.cat(eis, 1), gp, parts


def csr_order(ei):
    """The stable sort by target: position k of the CSR the kernels walk holds COO edge order[k]."""
    return torch.sort(ei[1], stable=True).indices


def degrees(name):
    ei, gp, _ = layout(name)
    N = gp[-1]
    return np.bincount(ei[1].numpy(), minlength=N), np.bincount(ei[0].numpy(), minlength=N)


# ---- which kernel instance a (shape, batch) pair selects: the launchers' conditions in plain Python --------------------------------
def fused_applicable(Fin, heads, Fh, E):      # gat_fused_applicable, gat_fused.hip
    return Fin in (32, 64) and Fh in (32, 64) and heads in (1, 2, 4) and Fin <= Fh and E > 0


def aggregate_instance(heads, Fh, N, E):      # launch_gat_aggregate, gat.hip: (NCH, DENSE)
    HF = heads * Fh
    assert HF <= 1024 and heads <= 32
    if HF <= 256:
        return 1, E > 4 * N
    return (2, False) if HF <= 512 else (4, False)


def da_row_blocks(N):                          # train_prologue, gat_bwd.hip
    return max(1, min(256, (N + 255) // 256))


# ---- layer shapes (Fin, heads, Fh) ---------------------------------------------------------------------------------------------------
FUSED_SHAPES = [(Fin, H, Fh) for Fin, Fh in ((32, 32), (32, 64), (64, 64)) for H in (1, 2, 4)]
GATHER_SHAPES = [(32, 4, 64), (36, 3, 20), (16, 8, 32), (4, 1, 4), (32, 1, 256), (32, 8, 64), (64, 6, 64), (32, 32, 32), (48, 5, 128)]
BWD_SHAPES = [(32, 4, 64), (36, 3, 20), (16, 8, 32), (64, 1, 256), (4, 1, 4), (64, 2, 32)]
BIG_SHAPES = [(32, 4, 64), (36, 3, 20)]
WIDE_HUB = ("dense", 32, 2, 16, 4.0, 2.0)      # (batch, Fin, heads, Fh, x scale, weight scale): the `wide` fixture on hubs, see NOTES.md
PLATEAU = ("plateau", 32, 2, 32, 1.0, 1.0)
PLATEAU_ZA, PLATEAU_ZB = 24.0, 1.0             # z = s + t of an A -> A and of a B -> B edge, both heads: e_A - e_B = 23


def _plateau_inputs(Fin, heads, Fh, W, a):
    """Rows with prescribed scores: z_h(x) = c_h . x with c_h = W_h^T (a_src + a_tgt) for an edge between equal rows, so
    x = pinv(C) z + (a part orthogonal to every c_h) has the score z on every head.  Group A: one row, bit-identical copies;
    group B: xb plus noise of 1e-3."""
    Wd, ad = W.double(), a.double()
    Cm = torch.stack([Wd[h * Fh:(h + 1) * Fh].t() @ (ad[h, :Fh] + ad[h, Fh:]) for h in range(heads)])        # (heads, Fin)
    pinv = torch.linalg.pinv(Cm)
    free = torch.from_numpy(O.formula_normal("gat64/plateau/free", (2, Fin), seed=5)).double()
    free = free - (free @ pinv) @ Cm                                                                             # C free^T = 0
    xa = pinv @ torch.full((heads,), PLATEAU_ZA, dtype=torch.float64) + free[0]
    xb = pinv @ torch.full((heads,), PLATEAU_ZB, dtype=torch.float64) + free[1]
    noise = torch.from_numpy(O.formula_normal("gat64/plateau/noise", (PLATEAU_N - PLATEAU_A, Fin), seed=6)).double() * 1e-3
    return torch.cat([xa.expand(PLATEAU_A, Fin), xb + noise], 0).float().contiguous()


@lru_cache(maxsize=None)
def inputs(bname, Fin, heads, Fh, concat, xs=1.0, ws=1.0):
    """X (N, Fin), W (heads * Fh, Fin), a (heads, 2 * Fh), R (N, Fout), edge masks (heads, E) in COO order, output mask (N, Fout),
    all fp32.  Weights are xavier_uniform with gain 1.414 (graph_attention.py:36-37) times ws; masks are nn.Dropout's at p = 0.3;
    the single in-edge of the first in-degree-1 row is masked out on every head."""
    ei, gp, _ = layout(bname)
    N, E, Fo = gp[-1], ei.shape[1], heads * Fh if concat else Fh
    tag = f"gat64/{bname}/{Fin}x{heads}x{Fh}"
    bw, ba = 1.414 * float(np.sqrt(6.0 / (Fin + Fh))) * ws, 1.414 * float(np.sqrt(6.0 / (2 * Fh + 1))) * ws
    W = torch.from_numpy(O.formula_uniform(tag + "/w", (heads * Fh, Fin), -bw, bw, 1))
    a = torch.from_numpy(O.formula_uniform(tag + "/a", (heads, 2 * Fh), -ba, ba, 2))
    if bname == "plateau":
        X = _plateau_inputs(Fin, heads, Fh, W, a)
    else:
        X = torch.from_numpy(O.formula_normal(tag + "/x", (N, Fin), seed=3)) * xs
    R = torch.from_numpy(O.formula_normal(tag + f"/r{concat}", (N, Fo), seed=4))
    em = O.dropout_mask_from_uniform(torch.from_numpy(O.formula_uniform(tag + "/em", (heads, E), 0.0, 1.0, 5)), P_DROP)
    om = O.dropout_mask_from_uniform(torch.from_numpy(O.formula_uniform(tag + f"/om{concat}", (N, Fo), 0.0, 1.0, 6)), P_DROP)
    lone = lone_masked_edge(bname)
    if lone is not None:
        em[:, lone] = 0.0
    return X, W, a, R, em, om


def lone_masked_edge(bname):
    """COO position of the only in-edge of the first in-degree-1 row (None: the batch has no such row)."""
    ei, gp, _ = layout(bname)
    ind = np.bincount(ei[1].numpy(), minlength=gp[-1])
    rows = np.flatnonzero(ind == 1)
    return int(np.flatnonzero(ei[1].numpy() == rows[0])[0]) if len(rows) else None


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def layer_run(parts, X, W, a, heads, Fh, concat, dt, R=None, em=None, om=None, exp=None, detach_max=False):
    """One multi-head layer on a batch by O.gat_head_forward per graph and head in dtype dt; with R also the gradients of
    sum_g (out_g * R_g).sum() with respect to X, W and a."""
    Xq, Wq, aq = (t.to(dt).clone().requires_grad_(R is not None) for t in (X, W, a))
    with oracle_with(exp, detach_max):
        outs = []
        for ei, lo, hi, e0, e1 in parts:
            hs = [O.gat_head_forward(Xq[lo:hi], ei, Wq[h * Fh:(h + 1) * Fh], aq[h:h + 1], ALPHA,
                                     None if em is None else em[h, e0:e1].reshape(-1, 1)) for h in range(heads)]
            outs.append(torch.cat(hs, 1) if concat else torch.stack(hs, 0).mean(0))
        out = torch.cat(outs, 0)
        if om is not None:
            out = out * om.to(dt)
        if R is None:
            return {"out": out.detach()}
        loss = sum((out[lo:hi] * R[lo:hi].to(dt)).sum() for _, lo, hi, _, _ in parts)
        loss.backward()
    return {"out": out.detach(), "dX": Xq.grad, "dW": Wq.grad, "da": aq.grad}


def _runs(bname, Fin, heads, Fh, concat, mode, xs, ws, **kw):
    X, W, a, R, em, om = inputs(bname, Fin, heads, Fh, concat, xs, ws)
    parts = layout(bname)[2]
    if mode == "eval":
        R = em = om = None
    elif mode == "grad":
        em = om = None
    return lambda dt, **k: layer_run(parts, X, W, a, heads, Fh, concat, dt, R, em, om, **k, **kw)


@lru_cache(maxsize=None)
def reference(bname, Fin, heads, Fh, concat, mode, xs=1.0, ws=1.0) -> GatRef:
    """mode `eval`: out; `grad`: out, dX, dW, da without masks; `train`: the same with the case's dropout masks."""
    run = _runs(bname, Fin, heads, Fh, concat, mode, xs, ws)
    return GatRef(run(torch.float64), run(torch.float32), run(torch.float32, exp=exp_fx))


def detached_max_gradients(bname, Fin, heads, Fh, concat, xs=1.0, ws=1.0):
    """The float64 gradients with the graph-wide max treated as a constant: what a backward without the max term computes."""
    return _runs(bname, Fin, heads, Fh, concat, "grad", xs, ws, detach_max=True)(torch.float64)


def edge_scores(bname, Fin, heads, Fh, dt, xs=1.0, ws=1.0):
    """e = LeakyReLU(a . [Wh_src || Wh_tgt]) of every edge and head (heads, E), graph_attention.py:53-65 in dtype dt.  The products are
    written as broadcast multiplies and row sums, so that a row's value does not depend on where a GEMM's blocking puts it: equal
    feature rows give equal scores on every machine, as they do in the kernels."""
    X, W, a = (t.to(dt) for t in inputs(bname, Fin, heads, Fh, 1, xs, ws)[:3])
    ei = layout(bname)[0]
    out = []
    for h in range(heads):
        hh = (X[:, None, :] * W[h * Fh:(h + 1) * Fh][None]).sum(2)
        out.append(torch.nn.functional.leaky_relu((torch.cat([hh[ei[0]], hh[ei[1]]], dim=1) * a[h:h + 1]).sum(1), ALPHA))
    return torch.stack(out)


# ---- the module path: widths that are padded (Fin 22 -> 24, Fh 6 -> 8, 5 -> 8) --------------------------------------------------------
MODULE_FIN = 22


def module_inputs(kind):
    """`layer`: MultiHeadGATLayer(22, 18, 3 heads, concat) ; `net`: GATNetwork(22, 6, 5, 1 head, 2 layers), on `general`, p = 0.3.
    (params as the state_dict of the network form, layer shapes [(Fin, Fh, heads, concat)], X, R, masks per layer)."""
    ei, gp, _ = layout("general")
    N, E = gp[-1], ei.shape[1]
    if kind == "layer":
        heads, shapes = 3, [(MODULE_FIN, 6, 3, True)]
        params = {f"gat_layers.0.heads.{h}.{n}": v for h in range(3) for n, v in
                  (("W.weight", _xavier(f"gat64/module/w{h}", (6, MODULE_FIN))), ("a.weight", _xavier(f"gat64/module/a{h}", (1, 12))))}
    else:
        heads, shapes = 1, [(MODULE_FIN, 6, 1, True), (6, 5, 1, False)]
        params = dict(O.make_gat_params(MODULE_FIN, 6, 5, 1, 2, seed=7))
    X = torch.from_numpy(O.formula_normal(f"gat64/module/{kind}/x", (N, MODULE_FIN), seed=3))
    Fo = shapes[-1][1] * (shapes[-1][2] if shapes[-1][3] else 1)
    R = torch.from_numpy(O.formula_normal(f"gat64/module/{kind}/r", (N, Fo), seed=4))
    masks, lone = [], lone_masked_edge("general")
    for l, (_, Fh, H, cat) in enumerate(shapes):
        em = O.dropout_mask_from_uniform(torch.from_numpy(O.formula_uniform(f"gat64/module/{kind}/em{l}", (H, E), 0.0, 1.0, 5)), P_DROP)
        om = O.dropout_mask_from_uniform(torch.from_numpy(O.formula_uniform(f"gat64/module/{kind}/om{l}", (N, Fh * H if cat else Fh), 0.0, 1.0, 6)), P_DROP)
        em[:, lone] = 0.0
        masks.append((em, om))
    return params, shapes, heads, X, R, masks


def _xavier(name, shape):
    b = 1.414 * float(np.sqrt(6.0 / (shape[0] + shape[1])))
    return torch.from_numpy(O.formula_uniform(name, shape, -b, b, 7))


def _module_run(kind, dt, exp=None):
    params, shapes, heads, X, R, masks = module_inputs(kind)
    ei = layout("general")[0]
    q = {k: v.to(dt).clone().requires_grad_(True) for k, v in params.items()}
    Xq = X.to(dt).clone().requires_grad_(True)
    with oracle_with(exp):
        if kind == "layer":     # a lone concat layer: gat_network_forward's first layer of two
            em, om = masks[0]
            hs = [O.gat_head_forward(Xq, ei, q[f"gat_layers.0.heads.{h}.W.weight"], q[f"gat_layers.0.heads.{h}.a.weight"], ALPHA,
                                     em[h].reshape(-1, 1)) for h in range(heads)]
            out = torch.cat(hs, 1) * om.to(dt)
        else:
            out = O.gat_network_forward(q, Xq, ei, heads, len(shapes), ALPHA, masks=masks)
        (out * R.to(dt)).sum().backward()
    res = {"out": out.detach(), "dX": Xq.grad}
    res.update({k: v.grad for k, v in q.items()})
    return res


@lru_cache(maxsize=None)
def module_reference(kind) -> GatRef:
    return GatRef(_module_run(kind, torch.float64), _module_run(kind, torch.float32), _module_run(kind, torch.float32, exp_fx))
