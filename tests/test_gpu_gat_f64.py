"""The graph attention kernels (csrc/gat.hip, gat_fused.hip, gat_bwd.hip) against float64 at hubs, wide layers and max ties: every
template instance of the aggregate-first schedule, the NCH 1 / 2 / 4 and DENSE instances of the gather schedule, rows and 4-row
segments of 63 / 64 / 65 / 129 in-edges, heads up to 32, batches whose graphs straddle segments and 32-node tiles around an edgeless
graph, the train-mode forward and the backward with dropout masks at both concat values and with three row blocks, the gradient
through the graph-wide max on a hub graph (one arg-max edge) and on a plateau (40 tied arg-max edges), the regrowth of the per-graph
max table inside a live context, and the module path at widths that are padded.

Cases, references and the bar are tests/gat_cases.py: err = max|got - ref64| / max|ref64| with no floor in the denominator,
bar = max(4 * dev32, 4 * devfx, 16 * eps32); dev32 and devfx are deviations of the fp32 oracle (plain, and with an fp32 model of
__expf) from the float64 oracle, computed on the CPU.  Rows without in-edges are exactly zero.  tests/test_gat_cases_host.py asserts
which branch each case reaches; NOTES.md ("GAT float64 bars") carries the table of the lines these tests print under -s."""
import os

import numpy as np
import pytest
import torch

import gat_cases as GC
import mgunet
from mgunet import _lib
from mgunet.gat import coo_to_csr_device

pytestmark = pytest.mark.gpu

_CTX, _GRAPH = {}, {}


def make_ctx(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Context(0)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def context(gather: bool):
    """One context per schedule for the whole file: the gather schedule is forced where the aggregate-first one would apply."""
    if gather not in _CTX:
        _CTX[gather] = make_ctx({"MGU_NO_GAT_FUSED": "1"} if gather else {})
    return _CTX[gather]


class Graph:
    """A batch on the device: CSR by target (stable), graph_ptr, the transposed CSR of the backward, the COO -> CSR edge order."""

    def __init__(self, bname, cuda):
        ei, gp, _ = GC.layout(bname)
        self.N, self.E, self.G = gp[-1], ei.shape[1], len(gp) - 1
        self.rowptr, self.col = coo_to_csr_device(ei.to(cuda), self.N)
        self.gp = torch.tensor(gp, dtype=torch.int32, device=cuda) if self.G > 1 else None
        self.rps = torch.empty(self.N + 1, dtype=torch.int32, device=cuda)
        self.eid, self.tgt = torch.empty(self.E, dtype=torch.int32, device=cuda), torch.empty(self.E, dtype=torch.int32, device=cuda)
        _lib.call("mgu_csr_transpose_device", cuda, self.rowptr, self.col, self.E, self.N, self.rps, self.eid, self.tgt)
        self.order = GC.csr_order(ei)
        self.no_in_edges = torch.from_numpy(np.bincount(ei[1].numpy(), minlength=self.N) == 0)


def graph(bname, cuda) -> Graph:
    if bname not in _GRAPH:
        _GRAPH[bname] = Graph(bname, cuda)
    return _GRAPH[bname]


def eval_forward(ctx, cuda, g, X, W, a, heads, Fh, concat):
    """mgu_gat_layer_forward_prepared three times (consecutive generations of the max table), then the one-shot entry: equal bytes."""
    Fin = X.shape[1]
    Xd, Wd, ad = X.to(cuda), W.to(cuda), a.to(cuda)
    prep = _lib.Prepared("mgu_gat_prepare", cuda, Wd, ad, heads, Fh, Fin, 1, ctx=ctx)
    res = []
    for _ in range(4):
        out = torch.full((g.N, heads * Fh if concat else Fh), float("nan"), device=cuda)
        if len(res) < 3:
            _lib.call("mgu_gat_layer_forward_prepared", cuda, prep.handle, Xd, g.N, g.rowptr, g.col, g.E, g.gp, g.G, concat, GC.ALPHA, out, ctx=ctx)
        else:
            _lib.call("mgu_gat_layer_forward", cuda, Xd, g.N, Fin, g.rowptr, g.col, g.E, g.gp, g.G, Wd, ad, heads, Fh, concat, GC.ALPHA, out, ctx=ctx)
        res.append(out)
    torch.cuda.synchronize()
    del prep
    assert all(torch.equal(res[0], r) for r in res[1:])
    return res[0].cpu()


def check_eval(ctx, cuda, bname, shape, concat, what):
    Fin, heads, Fh = shape
    g = graph(bname, cuda)
    X, W, a = GC.inputs(bname, Fin, heads, Fh, concat)[:3]
    got = eval_forward(ctx, cuda, g, X, W, a, heads, Fh, concat)
    GC.reference(bname, Fin, heads, Fh, concat, "eval").check("out", got, what=what)
    assert not got[g.no_in_edges].any()                          # rows without in-edges: ELU(0) of an empty sum, exactly 0
    return got


EVAL = [("fused", s) for s in GC.FUSED_SHAPES] + [("gather", s) for s in GC.GATHER_SHAPES]


@pytest.mark.parametrize("bname", ["dense", "sparse"])
@pytest.mark.parametrize("family,shape", EVAL, ids=[f"{f}-{'x'.join(map(str, s))}" for f, s in EVAL])
def test_eval_forward(cuda, family, shape, bname):
    """Aggregate-first: all nine (Fin, Fh, heads) instances.  Gather: NCH 1 (fast path 4 x 4 on `sparse`, 2 x 8 on `dense`, heads > 4,
    one head of width 256), NCH 2 and 4 full and partly filled.  Both on hubs of 129 in-edges and across an edgeless graph."""
    ctx = context(family == "gather")
    for concat in (0, 1):
        check_eval(ctx, cuda, bname, shape, concat, f"eval {family} {shape} `{bname}` concat {concat}")


def test_max_table_regrowth(cuda):
    """14 graphs x 32 heads = 448 (graph, head) maxima > the table's first 256 entries: the table is reallocated between two calls
    of a live context; the call that made it grow and a small case after it are still right, and the small case gives the bytes it
    gave before."""
    ctx = make_ctx({"MGU_NO_GAT_FUSED": "1"})
    small = ("sparse", (36, 3, 20), 1)
    before = check_eval(ctx, cuda, *small, "regrowth: (36, 3, 20) `sparse` before")
    check_eval(ctx, cuda, "many", (32, 32, 32), 1, "regrowth: (32, 32, 32) `many`")
    after = check_eval(ctx, cuda, *small, "regrowth: (36, 3, 20) `sparse` after")
    assert torch.equal(before, after)
    check_eval(context(False), cuda, "many", (32, 4, 32), 0, "regrowth: fused (32, 4, 32) `many`")     # 14 graphs inside one 32-node tile


def check_train(cuda, bname, shape, concat, modes, xs=1.0, ws=1.0, label=None):
    """mgu_gat_layer_forward_train and the backward (`train`: with the case's dropout masks, _backward_train; `grad`: no masks,
    mgu_gat_layer_backward): out, dX, dW, da at the bar, a second backward with the same bytes, no error word."""
    Fin, heads, Fh = shape
    ctx, g = context(False), graph(bname, cuda)
    X, W, a, R, em, om = GC.inputs(bname, Fin, heads, Fh, concat, xs, ws)
    Xd, Wd, ad, Rd = X.to(cuda), W.to(cuda), a.to(cuda), R.to(cuda)
    emd, omd = em[:, g.order].t().contiguous().to(cuda), om.to(cuda)        # (E, heads) in the CSR order of col[]
    for mode in modes:
        what = f"{label or mode} {shape} `{bname}` concat {concat}"
        ref = GC.reference(bname, Fin, heads, Fh, concat, mode, xs, ws)
        masks = (emd, omd) if mode == "train" else (None, None)
        out = torch.full_like(Rd, float("nan"))
        _lib.call("mgu_gat_layer_forward_train", cuda, Xd, g.N, Fin, g.rowptr, g.col, g.E, g.gp, g.G, Wd, ad, heads, Fh, concat, GC.ALPHA,
                  *masks, out, ctx=ctx)
        runs = []
        for _ in range(2):
            dX, dW, da = (torch.full_like(t, float("nan")) for t in (Xd, Wd, ad))
            args = (Xd, g.N, Fin, g.rowptr, g.col, g.E, g.rps, g.eid, g.tgt, g.gp, g.G, Wd, ad, heads, Fh, concat, GC.ALPHA)
            if mode == "train":
                _lib.call("mgu_gat_layer_backward_train", cuda, *args, *masks, Rd, dX, dW, da, ctx=ctx)
            else:
                _lib.call("mgu_gat_layer_backward", cuda, *args, Rd, dX, dW, da, ctx=ctx)
            runs.append((dX, dW, da))
        _lib.call("mgu_sync_check", cuda, ctx=ctx)                            # the max term found its edge
        ref.check("out", out, what=what)
        assert not out[g.no_in_edges.to(cuda)].any()                          # rows without in-edges: exactly 0
        for name, t in zip(("dX", "dW", "da"), runs[0]):
            ref.check(name, t, what=what)
        assert all(torch.equal(p, q) for p, q in zip(*runs)), what


@pytest.mark.parametrize("concat", [0, 1])
@pytest.mark.parametrize("shape", GC.BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_train_forward_backward(cuda, shape, concat):
    """`dense`: hubs of 129 in-edges and 75 out-edges, several graphs per wave of rows, an edgeless graph, a degree-1 row whose only
    edge is masked out; concat with several heads; head_sum at qh = 5."""
    check_train(cuda, "dense", shape, concat, ("train", "grad"))


@pytest.mark.parametrize("concat", [0, 1])
@pytest.mark.parametrize("shape", GC.BIG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_train_forward_backward_three_row_blocks(cuda, shape, concat):
    """`big` (646 nodes): gatb_da_partial_kernel with three row blocks, the last one ragged."""
    check_train(cuda, "big", shape, concat, ("train", "grad"))


@pytest.mark.parametrize("concat", [0, 1])
@pytest.mark.parametrize("case", [GC.WIDE_HUB, GC.PLATEAU], ids=["wide_hub", "plateau"])
def test_gradient_through_the_max(cuda, case, concat):
    """Inputs on which the 1e-10 of graph_attention.py:96 bites, so that the gradient through the graph-wide max carries a large
    share of dX, dW and da (tests/test_gat_cases_host.py: a backward without it is off by thousands of bars): `wide_hub` with one
    arg-max edge on head 1, `plateau` with 40 tied arg-max edges on both heads (gatb_max_term_kernel's serial walk)."""
    bname, Fin, heads, Fh, xs, ws = case
    check_train(cuda, bname, (Fin, heads, Fh), concat, ("grad",), xs, ws, label="wide_hub" if case is GC.WIDE_HUB else "plateau")


@pytest.mark.parametrize("kind", ["layer", "net"])
def test_module_path_padded_widths(cuda, kind):
    """MultiHeadGATLayer(22 -> 3 x 6, concat) and GATNetwork(22, 6, 5, 1 head, 2 layers) in train mode with injected masks on
    `general`: Fin 22 runs padded to 24, Fh 6 and 5 to 8, the output mask is padded with ones, gradients are sliced back."""
    params, shapes, heads, X, R, masks = GC.module_inputs(kind)
    ref = GC.module_reference(kind)
    ei = GC.layout("general")[0]
    if kind == "layer":
        mod = mgunet.MultiHeadGATLayer(GC.MODULE_FIN, 18, 3, GC.P_DROP, GC.ALPHA, concat=True)
        mod.load_state_dict({k[len("gat_layers.0."):]: v for k, v in params.items()})
        layers, prefix = [mod], "gat_layers.0."
    else:
        mod = mgunet.GATNetwork(GC.MODULE_FIN, 6, 5, 1, num_gat_layers=2, dropout_rate=GC.P_DROP, alpha=GC.ALPHA)
        mod.load_state_dict(params)
        layers, prefix = list(mod.gat_layers), ""
    mod = mod.to(cuda).train()
    for layer, m in zip(layers, masks):
        layer.dropout_masks = m
    Xd = X.to(cuda).requires_grad_(True)
    out = mod(Xd, ei.to(cuda))
    (out * R.to(cuda)).sum().backward()
    what = f"module {kind}"
    ref.check("out", out.detach(), what=what)
    ref.check("dX", Xd.grad, what=what)
    named = dict(mod.named_parameters())
    assert sorted(prefix + k for k in named) == sorted(params)
    for k, v in named.items():
        assert v.grad is not None, k
        ref.check(prefix + k, v.grad, what=what)
