"""Host-side mirror of model/gat/graph_attention.py routed through libmgunet.so.

Same classes, constructor signatures and state_dict() keys (`gat_layers.{l}.heads.{h}.W.weight`,
`...a.weight`).  forward(node_features, edge_index) takes the reference's COO int64 (2,E) edge_index;
the CSR-by-target the HIP kernels consume is derived once per edge_index tensor and cached.
All heads of a layer run in ONE kernel sequence (the reference loops over heads in Python,
graph_attention.py:151).  Train mode with dropout_rate > 0 (the reference's default 0.1: nn.Dropout on every head's
attention coefficients, :97, and on the layer output, :160) draws its masks on the device from the library's own
counter-based generator (mgu_dropout_mask; `mgunet.gat.seed_dropout(seed)` restarts the stream) -- or takes them from
`layer.dropout_masks = (edge_masks (H, E) in COO order, out_mask (N, F_out))`, the hook through which a test feeds the
same draw to the reference (tests/golden/gat_dropout.npz) -- and runs mgu_gat_layer_forward_train / _backward_train.
The layers are differentiable: when a parameter or the node features require grad, the call becomes a
torch.autograd.Function whose backward is mgu_gat_layer_backward (dX, dW, da per head), so the graph
branch trains under loss.backward() as in scripts/train_end_to_end.py:219-226, :478.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


def coo_to_csr_device(edge_index: torch.Tensor, num_nodes: int):
    """Stable COO -> CSR-by-target on the tensor's device (mgu_coo_to_csr_device: radix sort by target, callers cache the result).
    Ids outside [0, num_nodes) raise IndexError here, where the reference's h[edge_index[0]] would (graph_attention.py:57): ONE
    synchronisation per new edge_index tensor, none per forward."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must have shape (2, E)")
    if edge_index.dtype != torch.int64:
        raise TypeError("edge_index must be int64 (torch.long) like the reference's")
    _lib.require_hip(edge_index, "mgunet GAT")
    dev = edge_index.device
    ei = edge_index.contiguous()
    E = ei.shape[1]
    rowptr = torch.empty(num_nodes + 1, dtype=torch.int32, device=dev)
    col = torch.empty(E, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call("mgu_coo_to_csr_device", dev, ei if E else None, E, num_nodes, rowptr, col if E else None, status)
    if int(status.item()):
        raise IndexError(f"edge_index values must be in [0, {num_nodes})")
    return rowptr, col


class GraphAttentionLayer(nn.Module):
    """One attention head (graph_attention.py:5-118): parameter holder + single-head forward."""

    def __init__(self, in_features, out_features, dropout_rate, alpha, concat=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.dropout_rate, self.alpha, self.concat = dropout_rate, alpha, concat
        self.W = nn.Linear(in_features, out_features, bias=False)
        self.a = nn.Linear(2 * out_features, 1, bias=False)
        self.leakyrelu = nn.LeakyReLU(self.alpha)
        self.dropout = nn.Dropout(self.dropout_rate)
        nn.init.xavier_uniform_(self.W.weight, gain=1.414)  # :36-37
        nn.init.xavier_uniform_(self.a.weight, gain=1.414)

    def forward(self, node_features, edge_index, graph_ptr=None):
        return _gat_layer_forward([self], node_features, edge_index, True, self.alpha, self.training,
                                  self.dropout_rate, graph_ptr, _csr_cache(self), owner=self, out_dropout=False)


def _csr_cache(mod):
    c = mod.__dict__.get("_mgu_csr_cache")
    if c is None:
        c = {}
        mod.__dict__["_mgu_csr_cache"] = c
    return c


_context, _CTX = _lib.context, _lib._CTX   # the shared per-device contexts, under the names bench.py, tools/ and tests use


def stacked_head_weights(heads, cache):
    """(H*Fh4, Fin4) W panel and (H, 2*Fh4) a panel of a layer's heads, rebuilt only when a parameter changes.
    Fh4 = the per-head width rounded up to a multiple of 4 (16-byte lanes): the extra output features have zero weights
    and zero attention coefficients, so they are exactly ELU(0) = 0 and the caller slices them off."""
    sig = tuple((h.W.weight.data_ptr(), h.W.weight._version, h.a.weight.data_ptr(), h.a.weight._version) for h in heads)
    ent = cache.get("weights")
    if ent is None or ent[0] != sig:
        Fh = heads[0].out_features
        pad = (-Fh) % 4
        Ws = [F.pad(h.W.weight.detach(), (0, 0, 0, pad)) for h in heads]
        As = [torch.cat([F.pad(h.a.weight.detach()[:, :Fh], (0, pad)), F.pad(h.a.weight.detach()[:, Fh:], (0, pad))], 1) for h in heads]
        W = torch.cat(Ws, 0)
        a = torch.cat(As, 0).contiguous()
        if W.shape[1] % 4:
            W = F.pad(W, (0, 4 - W.shape[1] % 4))
        ent = cache["weights"] = (sig, W.contiguous(), a)
    return ent[1], ent[2]


def prepared_head_weights(heads, cache, dev, has_edges: bool):
    """mgu_gat_prepare once per (weight versions, device, has_edges): W^T a rows + fragment-order W^T (or the GEMM panel)."""
    W, a = stacked_head_weights(heads, cache)
    sig = (cache["weights"][0], str(dev), bool(has_edges))
    ent = cache.get("prepared")
    if ent is None or ent.key != sig:
        Fh = (heads[0].out_features + 3) // 4 * 4
        ent = cache["prepared"] = _lib.Prepared("mgu_gat_prepare", dev, W, a, len(heads), Fh, W.shape[1], 1 if has_edges else 0, key=sig)
    return ent.handle


_DROPOUT = {"seed": 0x6D67756E6574, "stream": 0}   # the library's dropout generator: one stream id per mask drawn


def seed_dropout(seed: int) -> None:
    """Restart the device-side dropout generator (train-mode GAT masks): the same seed gives the same masks call for call."""
    _DROPOUT["seed"], _DROPOUT["stream"] = int(seed) & (2 ** 64 - 1), 0


def _rank_key() -> int:
    """(rank of a data-parallel run, 0 otherwise): folded into the Philox key so that the ranks of one job draw DIFFERENT masks on
    their different shards from the same seed (torch's per-process generators differ the same way)."""
    try:
        import torch.distributed as dist
        return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
    except Exception:
        return 0


def _draw_mask(dev, shape, p: float) -> torch.Tensor:
    """nn.Dropout's mask (0 or 1 / (1 - p)) from Philox-4x32-10 on the device: element i of stream s under the key
    seed + 0x9E3779B97F4A7C15 * (rank, device index): ranks and devices of one process group never share a mask sequence."""
    m = torch.empty(shape, device=dev, dtype=torch.float32)
    _DROPOUT["stream"] += 1
    key = (_DROPOUT["seed"] + 0x9E3779B97F4A7C15 * (_rank_key() * 64 + (dev.index or 0))) & (2 ** 64 - 1)
    _lib.call("mgu_dropout_mask", dev, key, _DROPOUT["stream"], m.numel(), float(p), m)
    return m


def _gat_layer_forward(heads, X, edge_index, concat, alpha, training, dropout_rate, graph_ptr, cache, owner=None, out_dropout=True):
    _lib.require_hip(X, "mgunet GAT")
    if X.dtype != torch.float32:
        raise TypeError(f"expected float32 node features, got {X.dtype}")
    if X.dim() != 2:
        raise ValueError("node_features must be (N, F)")
    if heads[0].W.weight.shape[1] != X.shape[1]:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({X.shape[0]}x{X.shape[1]} and "
                           f"{heads[0].W.weight.shape[1]}x{heads[0].out_features})")
    params = [t for h in heads for t in (h.W.weight, h.a.weight)]
    train = training and dropout_rate > 0
    injected = getattr(owner, "dropout_masks", None) if train and owner is not None else None
    m = _LayerCall(heads, X, concat, alpha, cache, graph_ptr, edge_index=edge_index, with_perm=injected is not None)
    if train:   # a lone GraphAttentionLayer drops coefficients only (:97); :160 belongs to the multi-head layer
        return _GatLayerFn.apply(X, m, _dropout_masks(m, float(dropout_rate), injected, out_dropout), *params)
    if torch.is_grad_enabled() and (X.requires_grad or any(t.requires_grad for t in params)):
        # a node of the autograd graph whose backward is mgu_gat_layer_backward (gat_bwd.hip): loss.backward() reaches the GAT
        # parameters as it does in the reference's loop (scripts/train_end_to_end.py:219-226, :478)
        return _GatLayerFn.apply(X, m, None, *params)
    return _layer_forward(m, None)


class _LayerCall:
    """One layer call as the library takes it: the node features X (N, Fin) zero-padded to a multiple of 4 (exact: W is padded the
    same way in stacked_head_weights), the CSR by target (the module's cache of edge_index, or the caller's `csr`), graph_ptr, and
    the head width Fh padded to a multiple of 4 (narrow heads, e.g. the 2-segment predictor, run zero-padded and are sliced off)."""

    def __init__(self, heads, X, concat, alpha, cache, graph_ptr, edge_index=None, csr=None, with_perm=False):
        self.heads, self.concat, self.alpha, self.cache, self.dev = heads, 1 if concat else 0, float(alpha), cache, X.device
        self.N, self.Fin = X.shape
        self.H, self.Fh_true = len(heads), heads[0].out_features
        self.Fh = (self.Fh_true + 3) // 4 * 4
        self.W, self.a = stacked_head_weights(heads, cache)
        if self.W.device != self.dev:
            raise RuntimeError(f"GAT parameters are on {self.W.device}, node features on {self.dev}")
        Xc = X.detach().contiguous()
        self.X = F.pad(Xc, (0, 4 - self.Fin % 4)) if self.Fin % 4 else Xc
        if csr is None:
            self.rowptr, self.col, self.perm = _cached_csr(cache, edge_index, self.N, self.dev, with_perm)
        else:
            (self.rowptr, self.col), self.perm = csr, None
        self.E = self.col.numel()
        self.gp, self.G = None, 1
        if graph_ptr is not None:
            self.gp = graph_ptr.to(device=self.dev, dtype=torch.int32).contiguous()
            self.G = self.gp.numel() - 1


def _cached_csr(cache, edge_index, N, dev, with_perm):
    """(rowptr, col, perm): the CSR by target of edge_index, built once per edge_index tensor, and with_perm: the stable COO -> CSR
    edge permutation (the order mgu_coo_to_csr_device produces) that brings injected masks from COO order into CSR order."""
    key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, N, str(edge_index.device))
    ent = cache.get("csr")
    if ent is None or ent[0] != key:
        rowptr, col = coo_to_csr_device(edge_index.to(dev), N)
        ent = cache["csr"] = (key, rowptr, col, edge_index)  # keep the key tensor alive so data_ptr stays unique
        cache.pop("csr_t", None)
        cache.pop("perm", None)
    if not with_perm:
        return ent[1], ent[2], None
    pe = cache.get("perm")
    if pe is None or pe[0] != key:
        pe = cache["perm"] = (key, torch.sort(edge_index.to(dev)[1], stable=True).indices)
    return ent[1], ent[2], pe[1]


def _transposed_csr(cache, rowptr, col, N, dev):
    """CSR by source of the cached CSR by target (mgu_csr_transpose_device), built once per graph."""
    ent = cache.get("csr_t")
    if ent is None or ent[0] is not rowptr:
        E = col.numel()
        rp = torch.empty(N + 1, dtype=torch.int32, device=dev)
        eid = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        tgt = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        _lib.call("mgu_csr_transpose_device", dev, rowptr, col if E else None, E, N, rp, eid, tgt)
        ent = cache["csr_t"] = (rowptr, rp, eid, tgt)
    return ent[1], ent[2], ent[3]


def _dropout_masks(m, p, injected, out_dropout):
    """(edge mask (E, H) in CSR order, output mask at the padded width or None) of a train-mode call: drawn by mgu_dropout_mask,
    edge mask first, or injected as `layer.dropout_masks` = ((H, E) in COO order, (N, F_out) or None), the hook a test feeds the
    reference's draw through."""
    N, H, E = m.N, m.H, m.E
    Fo_true = H * m.Fh_true if m.concat else m.Fh_true
    if injected is not None:
        em_coo, om = injected
        if tuple(em_coo.shape) != (H, E) or (om is not None and tuple(om.shape) != (N, Fo_true)):
            raise ValueError(f"dropout_masks must be ((heads, E) = {(H, E)}, (N, F_out) = {(N, Fo_true)} or None)")
        edge_mask = em_coo.to(device=m.dev, dtype=torch.float32)[:, m.perm].t().contiguous()
        om = om.to(device=m.dev, dtype=torch.float32) if om is not None else None
    else:
        edge_mask = _draw_mask(m.dev, (max(E, 1), H), p)
        om = _draw_mask(m.dev, (N, Fo_true), p) if out_dropout else None
    if om is not None and m.Fh != m.Fh_true:   # heads run zero-padded to 16-byte lanes: the pad features are ELU(0) = 0 whatever their mask
        om = F.pad(om.view(N, -1, m.Fh_true), (0, m.Fh - m.Fh_true), value=1.0).reshape(N, -1)
    return edge_mask, om.contiguous() if om is not None else None


def _layer_forward(m, masks):
    """The layer through libmgunet: eval (masks None) on the prepared weights, train mode with explicit dropout masks."""
    out = torch.empty((m.N, m.H * m.Fh if m.concat else m.Fh), device=m.dev, dtype=torch.float32)
    col = m.col if m.E else None
    if masks is None:
        handle = prepared_head_weights(m.heads, m.cache, m.dev, m.E > 0)
        _lib.call("mgu_gat_layer_forward_prepared", m.dev, handle, m.X, m.N, m.rowptr, col, m.E, m.gp, m.G, m.concat, m.alpha, out)
    else:
        _lib.call("mgu_gat_layer_forward_train", m.dev, m.X, m.N, m.X.shape[1], m.rowptr, col, m.E, m.gp, m.G, m.W, m.a, m.H, m.Fh,
                  m.concat, m.alpha, *masks, out)
    if m.Fh != m.Fh_true:
        out = out.view(m.N, -1, m.Fh)[:, :, :m.Fh_true].reshape(m.N, -1).contiguous()
    return out


class _GatLayerFn(torch.autograd.Function):
    """One multi-head layer as a node of the autograd graph.  masks None: eval, backward mgu_gat_layer_backward; otherwise TRAIN mode
    with dropout (graph_attention.py:97, :160): mgu_gat_layer_forward_train and mgu_gat_layer_backward_train with the same masks."""

    @staticmethod
    def forward(ctx_, X, m, masks, *params):
        ctx_.m, ctx_.masks = m, masks
        return _layer_forward(m, masks)

    @staticmethod
    def backward(ctx_, gout):
        m = ctx_.m
        N, Fh, Fh_true = m.N, m.Fh, m.Fh_true
        g = gout.detach().float()
        if Fh != Fh_true:   # the padded output features never reach the caller: their gradient is 0
            g = F.pad(g.view(N, -1, Fh_true), (0, Fh - Fh_true)).reshape(N, -1)
        rps, eid, tgt = _transposed_csr(m.cache, m.rowptr, m.col, N, m.dev)
        dX = torch.empty_like(m.X) if ctx_.needs_input_grad[0] else None
        dW, da = torch.empty_like(m.W), torch.empty_like(m.a)
        args = (m.X, N, m.X.shape[1], m.rowptr, m.col if m.E else None, m.E, rps, eid, tgt, m.gp, m.G, m.W, m.a, m.H, Fh, m.concat, m.alpha)
        if ctx_.masks is None:
            _lib.call("mgu_gat_layer_backward", m.dev, *args, g.contiguous(), dX, dW, da)
        else:
            _lib.call("mgu_gat_layer_backward_train", m.dev, *args, *ctx_.masks, g.contiguous(), dX, dW, da)
        grads = []
        for h in range(m.H):
            grads.append(dW[h * Fh:h * Fh + Fh_true, :m.Fin].contiguous())
            grads.append(torch.cat([da[h:h + 1, :Fh_true], da[h:h + 1, Fh:Fh + Fh_true]], 1).contiguous())
        return (dX[:, :m.Fin].contiguous() if dX is not None else None, None, None, *grads)


class MultiHeadGATLayer(nn.Module):
    """graph_attention.py:120-160: all heads in one launch sequence; concat (:155) or mean (:158)."""

    def __init__(self, in_features, out_features, num_heads, dropout_rate, alpha, concat=True):
        super().__init__()
        self.num_heads, self.concat = num_heads, concat
        self.alpha, self.dropout_rate = alpha, dropout_rate
        if concat:
            assert out_features % num_heads == 0, "out_features must be divisible by num_heads if concatenating"
            self.head_out_features = out_features // num_heads
        else:
            self.head_out_features = out_features
        self.heads = nn.ModuleList(
            [GraphAttentionLayer(in_features, self.head_out_features, dropout_rate, alpha) for _ in range(num_heads)])
        self.dropout = nn.Dropout(dropout_rate)

    def forward(self, node_features, edge_index, graph_ptr=None):
        return _gat_layer_forward(list(self.heads), node_features, edge_index, self.concat, self.alpha,
                                  self.training, self.dropout_rate, graph_ptr, _csr_cache(self), owner=self)


class GATNetwork(nn.Module):
    """Drop-in for graph_attention.py:162-192 (same layer wiring, including the reference's
    multi-layer width mismatch: num_gat_layers >= 2 only works with num_heads == 1)."""

    def __init__(self, node_feature_dim, hidden_dim, output_dim, num_heads, num_gat_layers=1, dropout_rate=0.1,
                 alpha=0.2):
        super().__init__()
        self.num_gat_layers = num_gat_layers
        self.gat_layers = nn.ModuleList()
        if num_gat_layers == 1:
            self.gat_layers.append(MultiHeadGATLayer(node_feature_dim, output_dim, num_heads, dropout_rate, alpha, concat=False))
        else:
            self.gat_layers.append(MultiHeadGATLayer(node_feature_dim, hidden_dim, num_heads, dropout_rate, alpha, concat=True))
            for _ in range(num_gat_layers - 2):
                self.gat_layers.append(MultiHeadGATLayer(hidden_dim * num_heads, hidden_dim, num_heads, dropout_rate, alpha, concat=True))
            self.gat_layers.append(MultiHeadGATLayer(hidden_dim * num_heads, output_dim, num_heads, dropout_rate, alpha, concat=False))

    def forward(self, node_features, edge_index, graph_ptr=None):
        h = node_features
        for layer in self.gat_layers:
            h = layer(h, edge_index, graph_ptr)
        return h
