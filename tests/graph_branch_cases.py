"""Deterministic cases, float64 references and the error bar of the graph-branch kernels beyond the patch graph (csrc/ncut.hip,
losses.hip, region.hip, the CSR transpose of gat_bwd.hip).  Plain torch / numpy on the CPU, everything drawn from the oracle's
formula tensors: no fixture, no GPU.  Imported by tests/test_graph_branch_cases_host.py (case properties and the dev32 table, no
GPU) and tests/test_gpu_graph_branch_f64.py (the kernels against the same references).

The bar, the same rule for every tensor and scalar:

    err   = max|got - ref64| / max|ref64|          (no floor of 1 in the denominator; a scalar divides by |ref64|)
    dev32 = the same measure of the ORACLE RUN IN fp32 against the oracle run in float64: the reference's own arithmetic
    bar   = max(4 * dev32, 16 * eps32)

4: the kernels sum in another order than the reference; two fp32 orders are each about as far from float64 as the other and
neither bounds the other.  16 * eps32 (1.9e-6): the floor for a case where the fp32 oracle happens to land exactly.  Where ref64
is identically zero the result has to be exactly zero (err = inf otherwise)."""
from functools import lru_cache

import numpy as np
import torch

import mgunet_oracle as O

EPS32 = float(np.finfo(np.float32).eps)


def rel_err(got, ref64) -> float:
    """max|got - ref64| / max|ref64|; 0 / inf where ref64 is identically zero and got is / is not."""
    g = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    r = np.asarray(ref64.detach().cpu().numpy() if isinstance(ref64, torch.Tensor) else ref64, dtype=np.float64)
    assert g.shape == r.shape, (g.shape, r.shape)
    if r.size == 0:
        return 0.0
    d, m = float(np.abs(g - r).max()), float(np.abs(r).max())
    if not np.isfinite(d):
        return float("inf")
    if m == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / m


def bar_of(dev32: float) -> float:
    return max(4.0 * dev32, 16.0 * EPS32)


class Ref:
    """Float64 references of one case by name, and dev32 of each from the fp32 run of the same oracle code."""

    def __init__(self, r64: dict, r32: dict):
        self.r64 = {k: np.asarray(v.detach().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64) for k, v in r64.items()}
        self.dev32 = {k: rel_err(r32[k], self.r64[k]) for k in r64}

    def bar(self, name: str) -> float:
        return bar_of(self.dev32[name])

    def check(self, name: str, got, log=None, what="") -> float:
        """Assert got within the bar of the float64 reference `name`; returns the error (appended to `log` before the assert)."""
        err, bar = rel_err(got, self.r64[name]), self.bar(name)
        if log is not None:
            log.append((what, name, self.dev32[name], bar, err))
        print(f"  {what:40s} {name:8s} dev32 {self.dev32[name]:.1e}  bar {bar:.1e}  err {err:.1e}")
        assert err <= bar, (what, name, "err", err, "bar", bar, "dev32", self.dev32[name])
        return err


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
HUB_OUT, HUB_IN, LOOP, DUP = 3, 5, 7, (9, 11)


def general_graph(N: int, E: int, seed: int) -> torch.Tensor:
    """(2, E') int64 COO list on N >= 17 nodes, E >= 146: random sources and targets, then
      * node 3 is the source of edges 0..69 (out-degree >= 70: 17 full 4-edge batches and a tail), node 5 the target of 70..139;
      * edges 140, 141 are both the self-loop 7 -> 7, edges 142..145 four copies of 9 -> 11;
      * no edge leaves N-1 or N-3 and none enters N-2 or N-3: a node without out-edges, one without in-edges, an isolated one.
    The free end of the 140 hub edges is drawn below N-3, so the last rule takes nothing from the hubs."""
    assert N >= 17 and E >= 146
    u = O.formula_uniform("gbranch/graph", (2, E), 0.0, 1.0, seed).astype(np.float64)
    ei = np.minimum((u * N).astype(np.int64), N - 1)
    free = np.minimum((u * (N - 3)).astype(np.int64), N - 4)
    ei[0, 0:70], ei[1, 0:70] = HUB_OUT, free[1, 0:70]
    ei[0, 70:140], ei[1, 70:140] = free[0, 70:140], HUB_IN
    ei[:, 140:142] = LOOP
    ei[0, 142:146], ei[1, 142:146] = DUP
    keep = (ei[0] != N - 1) & (ei[0] != N - 3) & (ei[1] != N - 2) & (ei[1] != N - 3)
    return torch.from_numpy(np.ascontiguousarray(ei[:, keep]))


# ---- normalized cut ---------------------------------------------------------------------------------------------------------------
# tag: (N, D, K, E, unaligned feature view, logit shift of column 1, graph / data seed)
NCUT_CASES = {
    "g7": (37, 7, 3, 300, False, 0.0, 11),        # D % 4 != 0: ncut_node_kernel
    "g65": (101, 65, 5, 600, False, 0.0, 12),     # second column trip, second backward register
    "g130": (50, 130, 16, 400, False, 0.0, 13),   # widest K
    "g1000": (33, 1000, 2, 300, False, 0.0, 14),  # 16-lane kernel, 16 trips; last backward register partly filled
    "g1024": (19, 1024, 7, 200, False, 0.0, 19),  # the stated limit
    "g64": (200, 64, 2, 2000, False, 0.0, 16),    # headline width, mean degree 10
    "g64u": (50, 64, 4, 400, True, 0.0, 17),      # data_ptr() % 16 == 4: the fallback kernel at D % 4 == 0
    "k1": (17, 4, 1, 300, False, 0.0, 18),        # K = 1: the soft assignment is exactly 1
    "skip": (101, 65, 5, 600, False, -60.0, 12),  # g65 with segment 1 under the association threshold
}
SKIPPED = 1
GLOSS = 2.5      # upstream factor of the probabilities-leaf test
SIDE = 0.05      # weight of the (soft * R).sum() side loss of the logits-leaf test


def ncut_inputs(tag):
    """(edge_index (2, E'), X (N, D) fp32, logits (N, K) fp32, R (N, K) fp32, K, unaligned)."""
    N, D, K, E, unaligned, shift, seed = NCUT_CASES[tag]
    ei = general_graph(N, E, seed)
    X = torch.from_numpy(O.formula_normal("gbranch/ncut/x", (N, D), seed=seed)) / float(np.sqrt(D))
    L = torch.from_numpy(O.formula_normal("gbranch/ncut/l", (N, K), seed=seed + 100))
    if shift:
        L[:, SKIPPED] += shift
    R = torch.from_numpy(O.formula_normal("gbranch/ncut/r", (N, K), seed=seed + 200))
    return ei, X, L.contiguous(), R, K, unaligned


def unaligned_view(x: torch.Tensor) -> torch.Tensor:
    """The same (N, D) values as a contiguous view one float past a fresh allocation: data_ptr() % 16 == 4."""
    N, D = x.shape
    buf = torch.zeros(N * D + 4, dtype=x.dtype, device=x.device)
    v = buf[1:1 + N * D].view(N, D)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _ncut_prob_run(ei, X, L, K, dt):
    P = torch.softmax(L, dim=1).to(dt).requires_grad_(True)     # the fp32 softmax IS the input: both precisions start from it
    Xq = X.to(dt).requires_grad_(True)
    loss = O.normalized_cut_loss(Xq, ei, P, K)
    (GLOSS * loss).backward()
    with torch.no_grad():
        w = O.ncut_edge_weights(Xq, ei)
    return {"loss": loss.detach(), "dP": P.grad, "dX": Xq.grad, "w": w}


@lru_cache(maxsize=None)
def ncut_prob_reference(tag) -> Ref:
    """normalized_cut_loss with the soft assignments as the leaf, upstream factor GLOSS: loss, dP, dX and the edge weights."""
    ei, X, L, _, K, _ = ncut_inputs(tag)
    return Ref(_ncut_prob_run(ei, X, L, K, torch.float64), _ncut_prob_run(ei, X, L, K, torch.float32))


def _ncut_logit_run(ei, X, L, R, K, dt, skip_column):
    Lq, Xq = L.to(dt).requires_grad_(True), X.to(dt).requires_grad_(True)
    loss, soft, _ = O.mincut_forward(Xq, ei, K, Lq)
    (loss + SIDE * (soft * R.to(dt)).sum()).backward()
    out = {"loss": loss.detach(), "soft": soft.detach(), "dL": Lq.grad, "dX": Xq.grad}
    if skip_column:
        out["dL_skip"] = Lq.grad[:, SKIPPED]
    return out


@lru_cache(maxsize=None)
def ncut_logit_reference(tag) -> Ref:
    """MinCutRefinement.forward with the logits as the leaf plus the side loss SIDE * (soft * R).sum(): loss, soft, dlogits, dX;
    for `skip` also the skipped segment's gradient column as a tensor of its own (`dL_skip`, about 1e-26)."""
    ei, X, L, R, K, _ = ncut_inputs(tag)
    sk = NCUT_CASES[tag][5] != 0.0
    return Ref(_ncut_logit_run(ei, X, L, R, K, torch.float64, sk), _ncut_logit_run(ei, X, L, R, K, torch.float32, sk))


def ncut_assoc64(tag) -> np.ndarray:
    """assoc_k = sum_i P_ik deg_i in float64, P the case's fp32 softmax."""
    ei, X, L, _, K, _ = ncut_inputs(tag)
    X64, P = X.double(), torch.softmax(L, dim=1).double()
    w = O.ncut_edge_weights(X64, ei)
    deg = torch.zeros(X.shape[0], dtype=torch.float64).scatter_add_(0, ei[0], w)
    return (P * deg[:, None]).sum(0).numpy()


def ncut_loss_without(tag, skipped: int) -> float:
    """The float64 loss of the case with segment `skipped` left out of the sum."""
    ei, X, L, _, K, _ = ncut_inputs(tag)
    X64, P = X.double(), torch.softmax(L.double(), dim=1)
    w = O.ncut_edge_weights(X64, ei)
    deg = torch.zeros(X.shape[0], dtype=torch.float64).scatter_add_(0, ei[0], w)
    tot = 0.0
    for k in range(K):
        if k != skipped:
            tot += float((w * P[ei[0], k] * (1 - P[ei[1], k])).sum() / (P[:, k] * deg).sum())
    return tot


# ---- feature consistency ------------------------------------------------------------------------------------------------------------
# (B, N, D, margin): one lane group short of a row, D not a multiple of 64, two / three / five column trips, the grid stride
FEATCONS_CASES = [(1, 5, 4, 0.5), (2, 37, 20, 1.0), (3, 50, 68, 1.0), (2, 33, 132, 2.5), (1, 19, 260, 1.0), (3, 6000, 4, 0.5)]
FEATCONS_UP = 3.0


def featcons_inputs(case):
    B, N, D, margin = case
    s = 0.7 / float(np.sqrt(D))
    fu = torch.from_numpy(O.formula_normal("gbranch/fc/u", (B, N, D), seed=D)) * s
    fg = fu + torch.from_numpy(O.formula_normal("gbranch/fc/g", (B, N, D), seed=D + 1)) * s
    fg[0, 0] = fu[0, 0]                                          # a zero distance
    y = torch.from_numpy(O.formula_labels("gbranch/fc/y", (B, N), 2, seed=D + 2))
    return fu, fg, y, margin


def _featcons_run(fu, fg, y, margin, dt):
    a, b = fu.to(dt).requires_grad_(True), fg.to(dt).requires_grad_(True)
    v = O.feature_consistency_loss(a, b, y, margin)
    (FEATCONS_UP * v).backward()
    return {"value": v.detach(), "dfu": a.grad, "dfg": b.grad}


@lru_cache(maxsize=None)
def featcons_reference(case) -> Ref:
    fu, fg, y, margin = featcons_inputs(case)
    return Ref(_featcons_run(fu, fg, y, margin, torch.float64), _featcons_run(fu, fg, y, margin, torch.float32))


def featcons_hinge_share(case):
    """(share of rows with y == 0 and an active hinge, share of rows with y == 1)."""
    fu, fg, y, margin = featcons_inputs(case)
    dist = torch.sqrt(((fu.double() - fg.double()) ** 2).sum(2) + 1e-8)
    return float(((dist < margin) & (y == 0)).double().mean()), float((y == 1).double().mean())


# ---- dice ---------------------------------------------------------------------------------------------------------------------------
# (B, C, H, W): 1 class (zero gradient), 5 / 7 / 8 classes (the <8> kernels); 40 000 pixels > the 32 768 threads of the largest grid
DICE_CASES = [(2, 1, 23, 19), (2, 5, 23, 19), (2, 7, 23, 19), (2, 8, 23, 19), (1, 5, 200, 200)]
DICE_RAW = (2, 5, 23, 19)
DICE_RAW_PITCH, DICE_RAW_SCALE, DICE_RAW_SCALE_DEV, DICE_RAW_PREFILL = 8, 0.25, 2.0, 1e-4


def dice_inputs(case):
    B, C, H, W = case
    lg = torch.from_numpy(O.formula_normal("gbranch/dice/l", case, seed=C)) * 2
    y = torch.from_numpy(O.formula_labels("gbranch/dice/y", (B, H, W), C, seed=C + 1))
    return lg, y


def _dice_run(lg, y, dt):
    l = lg.to(dt).requires_grad_(True)
    v = O.dice_loss(l, y, 1.0)
    v.backward()
    return {"value": v.detach(), "grad": l.grad}


@lru_cache(maxsize=None)
def dice_reference(case) -> Ref:
    lg, y = dice_inputs(case)
    return Ref(_dice_run(lg, y, torch.float64), _dice_run(lg, y, torch.float32))


def dice_raw_prefill():
    """(B * HW, pitch) fp32 destination values of the gradient's own magnitude (1e-4), so that the accumulate check bites."""
    B, C, H, W = DICE_RAW
    return torch.from_numpy(O.formula_normal("gbranch/dice/pre", (B * H * W, DICE_RAW_PITCH), seed=3)) * DICE_RAW_PREFILL


@lru_cache(maxsize=None)
def dice_raw_reference() -> Ref:
    """Columns 0..C-1 of the destination after accumulate: prefill + grad_scale * (*grad_scale_dev) * dL/dlogits, rows = pixels."""
    B, C, H, W = DICE_RAW
    lg, y = dice_inputs(DICE_RAW)
    pre = dice_raw_prefill()[:, :C]
    k = DICE_RAW_SCALE * DICE_RAW_SCALE_DEV

    def run(dt):
        g = _dice_run(lg, y, dt)["grad"].permute(0, 2, 3, 1).reshape(B * H * W, C)
        return {"acc": pre.to(dt) + k * g}
    return Ref(run(torch.float64), run(torch.float32))


# ---- total variation ----------------------------------------------------------------------------------------------------------------
TV_SHAPE, TV_BIG, TV_WEIGHT, TV_UP = (2, 3, 9, 14), (2, 3, 11, 16), 0.7, 3.0


def tv_inputs(kind):
    """`nhwc`: (2, 3, 9, 14) values; `slice`: the (2, 3, 11, 16) tensor whose [:, :, 1:-1, 2:] is the input."""
    return torch.from_numpy(O.formula_normal("gbranch/tv/" + kind, TV_SHAPE if kind == "nhwc" else TV_BIG, seed=4))


def tv_slice(big):
    return big[:, :, 1:-1, 2:]


def _tv_run(x, dt):
    a = x.to(dt).contiguous().requires_grad_(True)
    v = O.tv_loss(a, TV_WEIGHT)
    (TV_UP * v).backward()
    return {"value": v.detach(), "grad": a.grad}


@lru_cache(maxsize=None)
def tv_reference(kind) -> Ref:
    x = tv_inputs(kind)
    x = x if kind == "nhwc" else tv_slice(x)
    return Ref(_tv_run(x, torch.float64), _tv_run(x, torch.float32))


# ---- region stage -------------------------------------------------------------------------------------------------------------------
# (B, Np, D, K): Np < the lane count; 4 dead threads (q = 6, 42 lanes); q = 25; one lane (npl = 1); several trips of every lane
POOL_CASES = [(1, 5, 4, 3), (2, 70, 24, 4), (3, 45, 100, 2), (1, 9, 1024, 5), (2, 1030, 64, 16)]
# (B, H, W, K, Cu, D)
FUSE_CASES = [(2, 37, 45, 3, 0, 4), (1, 50, 70, 2, 4, 8), (2, 33, 17, 5, 32, 64)]


def pool_inputs(case):
    """(feats (B*Np, D), labels (B*Np,) int64, empty segment of each image): segment b % K of image b is relabelled onto the next."""
    B, Np, D, K = case
    feats = torch.from_numpy(O.formula_normal("gbranch/pool/x", (B * Np, D), seed=D)) * 0.5
    lab = torch.from_numpy(O.formula_labels("gbranch/pool/y", (B, Np), K, seed=D + 1)).clone()
    empty = [b % K for b in range(B)]
    for b in range(B):
        lab[b][lab[b] == empty[b]] = (empty[b] + 1) % K
    return feats, lab.reshape(-1), empty


def _pool_run(feats, lab, B, Np, D, K, dt):
    out = torch.zeros(B * K, D, dtype=dt)
    f, l = feats.to(dt).reshape(B, Np, D), lab.reshape(B, Np)
    for b in range(B):
        for k in range(K):
            m = l[b] == k
            if int(m.sum()):
                out[b * K + k] = f[b][m].mean(0)
    return {"mean": out}


@lru_cache(maxsize=None)
def pool_reference(case) -> Ref:
    B, Np, D, K = case
    feats, lab, _ = pool_inputs(case)
    return Ref(_pool_run(feats, lab, B, Np, D, K, torch.float64), _pool_run(feats, lab, B, Np, D, K, torch.float32))


def fuse_inputs(case):
    """(f_u (B, Cu, H, W) or None, emb (B*K, D), labels (B*nph*npw,) int64 inside [0, K), nph, npw)."""
    B, H, W, K, Cu, D = case
    nph, npw = O.patch_grid(H, W, 16)
    fu = torch.from_numpy(O.formula_normal("gbranch/fuse/u", (B, Cu, H, W), seed=D)) if Cu else None
    emb = torch.from_numpy(O.formula_normal("gbranch/fuse/e", (B * K, D), seed=D + 1))
    lab = torch.from_numpy(O.formula_labels("gbranch/fuse/y", (B * nph * npw,), K, seed=D + 2))
    return fu, emb, lab, nph, npw


def fuse_reference(case) -> torch.Tensor:
    B, H, W, K, Cu, D = case
    fu, emb, lab, nph, npw = fuse_inputs(case)
    grid = emb.reshape(B, K, D)[torch.arange(B)[:, None], lab.reshape(B, nph * npw)]            # (B, Np, D)
    fg = torch.nn.functional.interpolate(grid.reshape(B, nph, npw, D).permute(0, 3, 1, 2), size=(H, W), mode="nearest")
    return torch.cat([fu, fg], 1) if fu is not None else fg


# ---- CSR transpose ------------------------------------------------------------------------------------------------------------------
CSR_CASES = [(203, 1500), (1, 3), (50, 0), (7, 3), (5000, 200000)]


def csr_edges(N, E) -> torch.Tensor:
    u = O.formula_uniform("gbranch/csr", (2, E), 0.0, 1.0, N).astype(np.float64)
    return torch.from_numpy(np.minimum((u * N).astype(np.int64), N - 1).reshape(2, E))
