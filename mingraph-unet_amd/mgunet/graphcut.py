"""Exact binary s-t min cut on the device (csrc/graphcut.hip): the solver of the energy that MinCutRefinement's constructor arguments
parameterise.  The reference documents gamma_unet_priors, sigma_intensity and sigma_features as the parameters of an energy E(S) "if
a solver was used" (model/graph_partition/mincut_refinement.py:9-25) and implements no solver; the energy below is THIS BUILD'S
definition, taken from that parameter documentation (as the node features of SURVEY 8a row L3 are):

    E(S) = sum_i D_i(S_i) + smoothness * sum_{(i,j) undirected} w_ij [S_i != S_j]
    D_i(fg) = -log p_i,   D_i(bg) = -log(1 - p_i),   p clamped to [1e-6, 1 - 1e-6]
    w_ij = exp(-(I_i - I_j)^2 / (2 sigma_intensity^2)) + gamma * exp(-|f_i - f_j|^2 / (2 sigma_features^2))

Either term of w_ij is dropped when its input is absent (with neither the edges carry no weight).  The terms are quantised to int32
capacities q(x) = min(lrintf(x * unit), 2^20), unit = 1024 by default, so the cut is an integer problem: the max-flow value and the
minimal sink side are unique, and labels, flow and round count are bit-reproducible.

    cut_capacities   prior (probabilities, or patch_labels' class counts) [+ intensity] [+ features] -> cap_source, cap_sink, cap_edge
    graph_cut        the cut of B graphs that share one topology: one workgroup per graph, the residual graph in LDS
    cut_energy       E(S) of any labelling in capacity units

Tie rule: a node is foreground (1, source side) iff the sink can NOT be reached from it in the residual graph of a maximum preflow.
That set is the same for every maximum preflow, so among cuts of equal cost the result is always the one with the largest foreground.
edge_index is the (2, E) int64 list of ONE graph and must hold both directions of every edge, no duplicate and no self loop
(ValueError otherwise); cap_edge follows its order, node i of graph b is row b*N + i, edge k of graph b is entry b*E + k.  A graph
must fit one workgroup's LDS: 20 N + 4 E + 40 bytes against the device's shared memory per block (160 KiB on gfx950: a 64 x 64
patch grid uses 143 KiB); a larger one is a ValueError naming the budget.

K labels (alpha-expansion over the same solver, one launch per batch):

    E(L) = sum_i U_i(L_i) + sum over pairs {i,j} of w_ij [L_i != L_j],   L_i in {0 .. K-1}
    U_i(k) = q(-log p_i(k)), p clamped to [1e-6, 1];   w_ij = cap_edge of the arc from the lower to the higher node id

    label_costs       class probabilities (or patch_labels' class counts, p = (n_k + 1) / (n_all + K)) -> U (B*N, K) int32
    graph_cut_multi   alpha = 0 .. K-1 cyclically; each move is one binary cut "node takes alpha" built and solved in LDS, accepted iff
                      it lowers E strictly; K rejected moves in a row end the loop
    cut_energy_multi  E(L) of any labelling

cap_edge is cut_capacities' (it does not depend on the prior); the direction from the higher to the lower id is not read (cut_capacities
writes both bitwise equal).  Costs and weights count as clamped to [0, 2^20].  For K = 2 with cap_source = U[:, 0] and cap_sink =
U[:, 1], E(L) is E(S).  LDS per graph: 20 N + 4 E + 48 + (N rounded up to 8) bytes -- 147 KiB for the 64 x 64 grid."""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import _lib
from .gat import coo_to_csr_device

_TOPOLOGY = OrderedDict()   # edge_index identity -> (rowptr, col, rev, perm, edge_index): derived once per tensor, like the CSR caches
_TOPOLOGY_SLOTS = 8


_WIDE = ("graph_cut_multi: a node of degree >= 4095: a move's 32-bit residual sink capacity can reach (1 + degree) * 2^20 and would "
         "overflow (the binary graph_cut takes such a graph)")


def _topology(edge_index: torch.Tensor, N: int, multi: bool = False):
    """CSR by source of one graph's edge list plus, per CSR position, the position of the reverse arc and the COO index (cached per
    edge_index tensor: ONE synchronisation per new tensor).  ValueError on a missing reverse edge, a duplicate edge or a self loop, and
    -- for the K-label functions only (multi) -- on a node of degree >= 4095, which the same pass finds."""
    if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
        raise ValueError("edge_index must be an int64 (2, E) tensor")
    _lib.require_hip(edge_index, "mgunet graph cut")
    dev = edge_index.device
    key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, N, str(dev))
    ent = _TOPOLOGY.get(key)
    if ent is not None:
        _TOPOLOGY.move_to_end(key)
        if multi and ent[6]:
            raise ValueError(_WIDE)
        return ent[:4]
    ei = edge_index.contiguous()
    E = ei.shape[1]
    rowptr, col = coo_to_csr_device(ei.flip(0), N)            # rows = sources, col = targets; IndexError on an id outside [0, N)
    rev = torch.empty(E, dtype=torch.int32, device=dev)
    perm = torch.empty(E, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("mgu_graphcut_rev_index", dev, ei if E else None, E, N, rowptr, col if E else None, rev if E else None, perm if E else None, status)
    st = int(status.item())
    if st & 15:
        what = [m for bit, m in ((1, "an edge without its reverse edge"), (2, "a duplicate edge"), (4, "a self loop"), (8, "an edge outside the graph"))
                if st & bit]
        raise ValueError("graph cut: edge_index holds " + ", ".join(what) + " (it must list both directions of every edge once)")
    _TOPOLOGY[key] = (rowptr, col, rev, perm, ei, edge_index, bool(st & 16))
    while len(_TOPOLOGY) > _TOPOLOGY_SLOTS:
        _TOPOLOGY.popitem(last=False)
    if multi and st & 16:
        raise ValueError(_WIDE)
    return rowptr, col, rev, perm


def _caps(t, n: int, what: str, dev) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != dev or t.numel() != n:
        raise ValueError(f"{what} must be an int32 tensor of {n} entries on the device of edge_index")
    return t.contiguous()


class GraphCut:
    """Result of graph_cut, all on the device: labels (B, N) uint8 (1 = foreground), flow (B,) int64 = E(labels) in capacity units,
    rounds (B,) int32, converged (B,) int32.  Nothing is read back until check()."""

    def __init__(self, labels, flow, rounds, converged, max_rounds):
        self.labels, self.flow, self.rounds, self.converged, self.max_rounds = labels, flow, rounds, converged, max_rounds

    def check(self) -> "GraphCut":
        """Synchronise and raise RuntimeError if a graph hit max_rounds before it converged (its labels are then no cut)."""
        bad = (self.converged == 0).nonzero().flatten().tolist()
        if bad:
            raise RuntimeError(f"graph_cut: graph(s) {bad} did not converge within max_rounds = {self.max_rounds}")
        return self


def graph_cut(edge_index, cap_source, cap_sink, cap_edge, num_nodes=None, batch=1, max_rounds=None, *, relabel_period=None,
              threads=None) -> GraphCut:
    """Min cut of `batch` graphs over one topology.  cap_source / cap_sink: int32 (batch * N) capacities of the arcs source -> node
    (cut when the node ends in the background) and node -> sink (cut when it ends in the foreground); cap_edge: int32 (batch * E) in
    edge_index order, each direction its own (negative values count as 0).  The inputs are not modified.  max_rounds (default
    8 N + 64) is a cap, not a tuning value: typical patch grids converge in tens of rounds, and hitting it is reported by
    GraphCut.converged / check(), never silently.  relabel_period / threads: the solver's global-relabel period and workgroup size
    (None: the measured defaults); the result does not depend on them.  No host read inside the call (beyond the
    one-off topology check of a new edge_index)."""
    B = int(batch)
    if B < 1:
        raise ValueError("batch must be positive")
    if not isinstance(cap_source, torch.Tensor):
        raise TypeError("capacities must be device tensors")
    N = int(num_nodes) if num_nodes is not None else cap_source.numel() // B
    if N < 1:
        raise ValueError("graph_cut needs at least one node")
    rowptr, col, rev, perm = _topology(edge_index, N)
    dev = edge_index.device
    E = edge_index.shape[1]
    cs, ct = _caps(cap_source, B * N, "cap_source", dev), _caps(cap_sink, B * N, "cap_sink", dev)
    ce = _caps(cap_edge, B * E, "cap_edge", dev) if E else None
    mr = 8 * N + 64 if max_rounds is None else int(max_rounds)
    if mr < 0:
        raise ValueError("max_rounds must not be negative")
    labels = torch.empty((B, N), dtype=torch.uint8, device=dev)
    flow = torch.empty(B, dtype=torch.int64, device=dev)
    rounds = torch.empty(B, dtype=torch.int32, device=dev)
    conv = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.call("mgu_graphcut_solve", dev, B, N, E, rowptr, col if E else None, rev if E else None, perm if E else None, cs, ct, ce, mr,
              int(relabel_period or 0), int(threads or 0), labels, flow, rounds, conv)
    return GraphCut(labels, flow, rounds, conv, mr)


def cut_capacities(prior, edge_index, intensity=None, features=None, *, counts_foreground=None, gamma=0.5, sigma_intensity=10.0,
                   sigma_features=1.0, smoothness=1.0, unit=1024, batch=1):
    """The energy's integer capacities -> (cap_source (B*N,), cap_sink (B*N,), cap_edge (B*E,)) int32.  prior: float32 (B*N) foreground
    probabilities, or -- with counts_foreground = the foreground class -- int32 (B*N, C) / (B, N, C) class counts as
    patch_labels(return_counts=True) gives them, turned into p = (n_fg + 1) / (n_all + 2) in the kernel.  intensity: optional float32
    (B*N) on the 0..255 scale of patch_features_u8; features: optional float32 (B*N, D).  cap_edge is bitwise symmetric."""
    B = int(batch)
    if not isinstance(prior, torch.Tensor):
        raise TypeError("prior must be a device tensor")
    dev = prior.device
    _lib.require_hip(prior, "mgunet.cut_capacities")
    if counts_foreground is None:
        if prior.dtype != torch.float32:
            raise TypeError("prior must be float32 probabilities (or int32 class counts with counts_foreground=)")
        rows, C, fg = prior.numel(), 0, 0
        p, cnt = prior.contiguous(), None
    else:
        if prior.dtype != torch.int32 or prior.dim() < 2:
            raise TypeError("class counts must be an int32 (B*N, C) or (B, N, C) tensor")
        C, fg = prior.shape[-1], int(counts_foreground)
        if not 0 <= fg < C:
            raise ValueError(f"counts_foreground {fg} outside the {C} counted classes")
        rows = prior.numel() // C
        p, cnt = None, prior.contiguous()
    if B < 1 or rows < B or rows % B:
        raise ValueError(f"{rows} prior rows do not split into {B} graphs")
    N = rows // B
    _topology(edge_index, N)                                  # ids in range, both directions present
    if edge_index.device != dev:
        raise ValueError("prior and edge_index must be on the same device")
    ei = edge_index.contiguous()
    E = ei.shape[1]
    D = 0
    for t, what in ((intensity, "intensity"), (features, "features")):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev):
            raise TypeError(f"{what} must be a float32 tensor on the prior's device")
    if intensity is not None:
        if intensity.numel() != rows:
            raise ValueError(f"intensity must have {rows} entries")
        intensity = intensity.contiguous()
    if features is not None:
        if features.numel() == 0 or features.numel() % rows:
            raise ValueError(f"features must be ({rows}, D)")
        features = features.reshape(rows, -1).contiguous()
        D = features.shape[1]
    if not (unit > 0 and smoothness >= 0 and sigma_intensity > 0 and sigma_features > 0):
        raise ValueError("unit and the sigmas must be positive, smoothness >= 0")
    cs = torch.empty(rows, dtype=torch.int32, device=dev)
    ct = torch.empty(rows, dtype=torch.int32, device=dev)
    ce = torch.empty(B * E, dtype=torch.int32, device=dev)
    _lib.call("mgu_graphcut_capacities", dev, B, N, ei if E else None, E, p, cnt, C, fg, intensity, features, D, float(gamma),
              float(sigma_intensity), float(sigma_features), float(smoothness), float(unit), cs, ct, ce if E else None)
    return cs, ct, ce


def cut_energy(labels, edge_index, cap_source, cap_sink, cap_edge, batch=1) -> torch.Tensor:
    """E(S) of a labelling (B, N) / (B*N,), any integer or bool dtype, non-zero = foreground, in capacity units -> int64 (B,): cap_sink
    over the foreground, cap_source over the background, cap_edge over the edges from foreground to background.  For the labels
    of graph_cut it equals GraphCut.flow; for any other labelling it is at least that."""
    B = int(batch)
    if not isinstance(labels, torch.Tensor) or labels.is_floating_point():
        raise TypeError("labels must be an integer device tensor")
    _lib.require_hip(labels, "mgunet.cut_energy")
    dev = labels.device
    if B < 1 or labels.numel() < B or labels.numel() % B:
        raise ValueError(f"{labels.numel()} labels do not split into {B} graphs")
    N = labels.numel() // B
    _topology(edge_index, N)
    E = edge_index.shape[1]
    lab = (labels != 0).to(torch.uint8).contiguous()
    cs, ct = _caps(cap_source, B * N, "cap_source", dev), _caps(cap_sink, B * N, "cap_sink", dev)
    ce = _caps(cap_edge, B * E, "cap_edge", dev) if E else None
    out = torch.empty(B, dtype=torch.int64, device=dev)
    _lib.call("mgu_graphcut_energy", dev, B, N, edge_index.contiguous() if E else None, E, lab, cs, ct, ce, out)
    return out


# ---- K labels --------------------------------------------------------------------------------------------------------------------
class MultiCut:
    """Result of graph_cut_multi, all on the device: labels (B, N) uint8, energy (B,) int64 = E(labels) in capacity units, moves,
    accepted, rounds (summed over the moves), converged: (B,) int32.  Nothing is read back until check()."""

    def __init__(self, labels, energy, moves, accepted, rounds, converged, max_cycles, max_rounds):
        self.labels, self.energy, self.moves, self.accepted, self.rounds, self.converged = labels, energy, moves, accepted, rounds, converged
        self.max_cycles, self.max_rounds = max_cycles, max_rounds

    def check(self) -> "MultiCut":
        """Synchronise and raise RuntimeError if a graph reached max_cycles, or a move of it max_rounds, before the expansion converged
        (its labels are then the last accepted labelling, not a local minimum)."""
        bad = (self.converged == 0).nonzero().flatten().tolist()
        if bad:
            raise RuntimeError(f"graph_cut_multi: graph(s) {bad} did not converge within max_cycles = {self.max_cycles} "
                               f"(max_rounds = {self.max_rounds} per move)")
        return self


def _costs(costs, B: int, what: str):
    """-> (contiguous (B*N, K) int32 costs, N, K)"""
    if not isinstance(costs, torch.Tensor):
        raise TypeError(f"{what}: costs must be a device tensor")
    _lib.require_hip(costs, what)
    if costs.dtype != torch.int32:
        raise TypeError(f"{what}: costs must be int32 (label_costs gives them), got {costs.dtype}")
    if costs.dim() not in (2, 3):
        raise ValueError(f"{what}: costs must be (B*N, K) or (B, N, K)")
    K = costs.shape[-1]
    if not 1 <= K <= 255:
        raise ValueError(f"{what}: {K} labels, a label is one byte: 1 <= K <= 255")
    rows = costs.numel() // K
    if B < 1 or rows < B or rows % B:
        raise ValueError(f"{what}: {rows} cost rows do not split into {B} graphs")
    return costs.reshape(rows, K).contiguous(), rows // B, K


def label_costs(prior, batch=1, unit=1024) -> torch.Tensor:
    """U (B*N, K) int32 = q(-log p), p clamped to [1e-6, 1].  prior: float32 (B*N, K) class probabilities, or int32 (B*N, K) /
    (B, N, K) class counts as patch_labels(return_counts=True) gives them, p = (n_k + 1) / (n_all + K).  One launch, evaluated in
    double: the count path is exact."""
    B = int(batch)
    if not isinstance(prior, torch.Tensor):
        raise TypeError("prior must be a device tensor")
    _lib.require_hip(prior, "mgunet.label_costs")
    if prior.dtype == torch.float32:
        if prior.dim() != 2:
            raise ValueError("class probabilities must be a float32 (B*N, K) tensor")
    elif prior.dtype == torch.int32:
        if prior.dim() not in (2, 3):
            raise ValueError("class counts must be an int32 (B*N, K) or (B, N, K) tensor")
    else:
        raise TypeError(f"prior must be float32 probabilities or int32 class counts, got {prior.dtype}")
    K = prior.shape[-1]
    if not 1 <= K <= 255:
        raise ValueError(f"label_costs: {K} labels, a label is one byte: 1 <= K <= 255")
    rows = prior.numel() // K
    if B < 1 or rows < B or rows % B:
        raise ValueError(f"{rows} prior rows do not split into {B} graphs")
    if not unit > 0:
        raise ValueError("unit must be positive")
    p = prior.contiguous()
    out = torch.empty((rows, K), dtype=torch.int32, device=prior.device)
    is_prob = prior.dtype == torch.float32
    _lib.call("mgu_graphcut_label_costs", prior.device, rows, K, p if is_prob else None, None if is_prob else p, float(unit), out)
    return out


def graph_cut_multi(edge_index, costs, cap_edge, batch=1, init=None, max_cycles=None, max_rounds=None, *, relabel_period=None,
                    threads=None) -> MultiCut:
    """Alpha-expansion of `batch` graphs over one topology, the whole loop in one launch.  costs: int32 (batch * N, K) (or (batch, N, K)),
    1 <= K <= 255; cap_edge: int32 (batch * E) in edge_index order, of which the arc from the lower to the higher node id is the
    pair's weight.  init: optional uint8 (batch, N) start labels (a value >= K is replaced by the node's cheapest label); None: every
    node's cheapest label, the lowest on ties.  max_cycles (default 32) and max_rounds (per move, default 8 N + 64) are caps, not tuning
    values: reaching one is reported by MultiCut.converged / check(), and the labels are then the last accepted labelling.
    relabel_period / threads as in graph_cut: they change nothing but `rounds`.  The inputs are not modified; no host read inside the
    call (beyond the one-off topology check of a new edge_index).  ValueError for a graph beyond one workgroup's LDS or with a node
    of degree >= 4095."""
    B = int(batch)
    U, N, K = _costs(costs, B, "graph_cut_multi")
    dev = U.device
    if isinstance(edge_index, torch.Tensor) and edge_index.device != dev:
        raise ValueError("costs and edge_index must be on the same device")
    rowptr, col, rev, perm = _topology(edge_index, N, multi=True)
    E = edge_index.shape[1]
    ce = _caps(cap_edge, B * E, "cap_edge", dev) if E else None
    if init is not None:
        if not isinstance(init, torch.Tensor) or init.dtype != torch.uint8 or init.device != dev or init.numel() != B * N:
            raise TypeError(f"init must be a uint8 tensor of {B * N} labels on the device of edge_index")
        init = init.contiguous()
    mc = 32 if max_cycles is None else int(max_cycles)
    mr = 8 * N + 64 if max_rounds is None else int(max_rounds)
    if mc < 0 or mr < 0:
        raise ValueError("max_cycles and max_rounds must not be negative")
    labels = torch.empty((B, N), dtype=torch.uint8, device=dev)
    energy = torch.empty(B, dtype=torch.int64, device=dev)
    moves, accepted, rounds, conv = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(4))
    _lib.call("mgu_graphcut_expand", dev, B, N, E, K, rowptr, col if E else None, rev if E else None, perm if E else None, U, ce, init, mc, mr,
              int(relabel_period or 0), int(threads or 0), labels, energy, moves, accepted, rounds, conv)
    return MultiCut(labels, energy, moves, accepted, rounds, conv, mc, mr)


def cut_energy_multi(labels, edge_index, costs, cap_edge, batch=1) -> torch.Tensor:
    """E(L) of a labelling (B, N) / (B*N,), any integer dtype with values in [0, K), in capacity units -> int64 (B,).  For the labels
    of graph_cut_multi it equals MultiCut.energy."""
    B = int(batch)
    if not isinstance(labels, torch.Tensor) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise TypeError("labels must be an integer device tensor")
    _lib.require_hip(labels, "mgunet.cut_energy_multi")
    U, N, K = _costs(costs, B, "cut_energy_multi")
    dev = labels.device
    if U.device != dev or labels.numel() != B * N:
        raise ValueError(f"labels must hold {B * N} entries on the device of costs")
    _topology(edge_index, N)
    E = edge_index.shape[1]
    lab = labels.clamp(0, 255).to(torch.uint8).contiguous()
    ce = _caps(cap_edge, B * E, "cap_edge", dev) if E else None
    out = torch.empty(B, dtype=torch.int64, device=dev)
    _lib.call("mgu_graphcut_energy_multi", dev, B, N, edge_index.contiguous() if E else None, E, K, lab, U, ce, out)
    return out
