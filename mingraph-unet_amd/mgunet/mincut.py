"""Host-side mirror of the MinCut stage of the patch-graph branch, routed through libmgunet.so:

* `MinCutRefinement` -- model/graph_partition/mincut_refinement.py:5-205: same constructor, `compute_edge_weights_for_ncut`,
  `normalized_cut_loss`, `forward(features, edge_index, K, segment_predictor_network)` -> `(loss, soft_assignments)`;
* `PatchSegmentPredictor` -- scripts/train_end_to_end.py:40-70: same constructor and state_dict() keys
  (`gnn_predictor.gat_layers...` or `mlp_predictor.{0,2}.{weight,bias}`).

The loss is a node of the autograd graph when its inputs require gradients: `loss.backward()` (train_end_to_end.py:472-479)
runs `mgu_ncut_backward` (gradients w.r.t. the segment logits / soft assignments AND the node features, through the edge
weights, as the reference's autograd does) and, for the MLP predictor, the Linear layers' data / weight gradients on the
library's 1x1-convolution backward kernels.  Under `torch.no_grad()` nothing is recorded.
The reference sums the weighted degree over the SOURCE index of the COO list (:96), so the kernels take a CSR by
source; it is derived once per edge_index tensor and cached, like the GAT's CSR by target.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from .gat import GATNetwork, coo_to_csr_device


def _check_features(x: torch.Tensor, what: str) -> None:
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{what} must be a (N, D) tensor")
    _lib.require_hip(x, "mgunet MinCut")
    if x.dtype != torch.float32:
        raise TypeError(f"expected float32 {what}, got {x.dtype}")


def _linear_run(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, relu: bool) -> torch.Tensor:
    """y = x W^T + b (optionally ReLU) as a 1x1 convolution over an (N, 1) image: the MFMA implicit-GEMM kernel.
    Returns the (N, ceil4(Cout)) buffer (pad columns are zero)."""
    N, Cin = x.shape
    Cout = w.shape[0]
    if Cin % 4:
        raise ValueError("MLP predictor widths must be multiples of 4 (16-byte NHWC pixels)")
    ld = (Cout + 3) // 4 * 4
    out = torch.empty((N, ld), device=x.device, dtype=torch.float32)
    _lib.call("mgu_conv2d_nhwc", x.device, x, 1, N, 1, Cin, w, b, None, None, Cout, 1, 1 if relu else 0, out, ld, 0)
    return out


class _LinearFn(torch.autograd.Function):
    """nn.Linear (+ ReLU) of the MLP segment predictor (train_end_to_end.py:59-63) with its backward on the HIP path:
    dX = dZ W (mgu_conv2d_dgrad_nhwc, k = 1), dW = dZ^T X (mgu_conv2d_wgrad_nhwc), db = column sums of dZ, dZ = dY where Y > 0."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        xc, w, b = x.detach().contiguous(), weight.detach().contiguous(), bias.detach().contiguous()
        y = _linear_run(xc, w, b, relu)
        ctx.relu, ctx.cout = relu, w.shape[0]
        ctx.save_for_backward(xc, w, y)
        return y[:, :w.shape[0]]

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        dev = x.device
        N, Cin = x.shape
        Cout, ld = ctx.cout, y.shape[1]
        dz = torch.zeros((N, ld), device=dev, dtype=torch.float32)
        dz[:, :Cout] = gy
        dx = torch.empty((N, Cin), device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        db = None
        if ctx.relu:
            _lib.call("mgu_relu_backward", dev, dz, y, dz.numel(), dz)
        if dx is not None:
            _lib.call("mgu_conv2d_dgrad_nhwc", dev, dz, w, 1, N, 1, Cin, Cout, 1, dx, Cin)
        if dw is not None:
            _lib.call("mgu_conv2d_wgrad_nhwc", dev, x, Cin, dz, 1, N, 1, Cin, Cout, 1, dw)
        if ctx.needs_input_grad[2]:
            dbp = torch.empty(ld, device=dev, dtype=torch.float32)
            _lib.call("mgu_channel_sum_nhwc", dev, dz, ld, N, ld, dbp)
            db = dbp[:Cout]
        return dx, dw, db, None


class _NcutFn(torch.autograd.Function):
    """normalized_cut_loss / MinCutRefinement.forward as one autograd node: forward mgu_ncut_forward, backward mgu_ncut_backward."""

    @staticmethod
    def forward(ctx, feats, assign, mod, edge_index, K, is_logits):
        loss, soft, hard = mod._ncut_run(feats, edge_index, assign, K, is_logits)
        P = soft if is_logits else assign.detach().to(torch.float32).contiguous()
        ctx.mod, ctx.edge_index, ctx.K, ctx.is_logits = mod, edge_index, K, is_logits
        ctx.save_for_backward(feats.detach().contiguous(), P)
        if is_logits:
            ctx.mark_non_differentiable(hard)
            return loss, soft, hard
        return loss

    @staticmethod
    def backward(ctx, gloss, gsoft=None, ghard=None):
        f, P = ctx.saved_tensors
        dev = f.device
        N, D = f.shape
        K = ctx.K
        rp_s, col_t = ctx.mod._csr_by_source(ctx.edge_index, N, dev)
        rp_t, col_s = ctx.mod._csr_by_target(ctx.edge_index, N, dev)
        E = col_t.numel()
        gl = gloss.detach().to(torch.float32).reshape(1).contiguous()
        gs = gsoft.detach().to(torch.float32).contiguous() if (ctx.is_logits and gsoft is not None) else None
        dA = torch.empty((N, K), device=dev, dtype=torch.float32)
        dF = torch.empty((N, D), device=dev, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        _lib.call("mgu_ncut_backward", dev, f, N, D, rp_s, col_t if E else None, rp_t, col_s if E else None, E, P, K, 1 if ctx.is_logits else 0,
                  gl, gs, dA, dF)
        return dF, (dA if ctx.needs_input_grad[1] else None), None, None, None, None


class PatchSegmentPredictor(nn.Module):
    """train_end_to_end.py:40-70: logits (N, num_segments) from the GAT-refined patch features."""

    def __init__(self, in_dim, num_segments, hidden_dim=None, use_gnn=False, num_gnn_layers=1, num_heads=1):
        super().__init__()
        self.use_gnn = use_gnn
        self.in_dim, self.num_segments = in_dim, num_segments
        if use_gnn:
            self.gnn_predictor = GATNetwork(node_feature_dim=in_dim, hidden_dim=hidden_dim if hidden_dim else in_dim,
                                            output_dim=num_segments, num_heads=num_heads, num_gat_layers=num_gnn_layers,
                                            dropout_rate=0.1, alpha=0.2)  # :46-54
        else:
            if hidden_dim is None:
                hidden_dim = in_dim * 2  # :57
            self.mlp_predictor = nn.Sequential(nn.Linear(in_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, num_segments))

    def _linear(self, x: torch.Tensor, lin: nn.Linear, relu: bool) -> torch.Tensor:
        if torch.is_grad_enabled() and (x.requires_grad or lin.weight.requires_grad or lin.bias.requires_grad):
            return _LinearFn.apply(x, lin.weight, lin.bias, relu)
        return _linear_run(x.detach().contiguous(), lin.weight.detach().contiguous(), lin.bias.detach().contiguous(), relu)[:, :lin.out_features]

    def forward(self, x, edge_index=None):
        _check_features(x, "x")
        if self.use_gnn:
            if edge_index is None:
                raise ValueError("edge_index must be provided for GNN-based segment predictor.")  # :66-67
            return self.gnn_predictor(x, edge_index)
        h = self._linear(x, self.mlp_predictor[0], relu=True)   # no dropout in the MLP branch: train == eval
        return self._linear(h.contiguous(), self.mlp_predictor[2], relu=False).contiguous()


class MinCutRefinement(nn.Module):
    """mincut_refinement.py:5-205.  The constructor arguments parameterise the energy E(S) of a solver the reference
    never implements (:9-16).  Here `solve` / `refine_patches` minimise that energy exactly with them (mgunet.graphcut: this build's
    definition of E(S), taken from the reference's parameter documentation) and `solve_multi` / `refine_patches_multi` its K-label form
    by alpha-expansion; the normalized-cut loss below does not use them."""

    def __init__(self, gamma_unet_priors=0.5, sigma_intensity=10.0, sigma_features=1.0):
        super().__init__()
        self.gamma_unet_priors = gamma_unet_priors
        self.sigma_intensity = sigma_intensity
        self.sigma_features = sigma_features
        self._csr = None

    def _csr_by_source(self, edge_index: torch.Tensor, N: int, dev):
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, N, str(dev))
        if self._csr is None or self._csr[0] != key:
            rowptr, col = coo_to_csr_device(edge_index.to(dev).flip(0), N)   # rows = sources, col = targets
            self._csr = (key, rowptr, col, edge_index)
        return self._csr[1], self._csr[2]

    def _csr_by_target(self, edge_index: torch.Tensor, N: int, dev):
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, N, str(dev))
        ent = self.__dict__.get("_csr_t")
        if ent is None or ent[0] != key:
            rowptr, col = coo_to_csr_device(edge_index.to(dev), N)   # rows = targets, col = sources (the backward's second gather)
            ent = self.__dict__["_csr_t"] = (key, rowptr, col, edge_index)
        return ent[1], ent[2]

    def solve(self, prior, edge_index, intensity=None, features=None, batch=1, smoothness=1.0, counts_foreground=None):
        """Exact min cut of E(S) (mgunet.graphcut) for `batch` graphs over edge_index, with gamma_unet_priors, sigma_intensity and
        sigma_features as the energy's gamma and sigmas.  prior: float32 (B*N) foreground probabilities (or int32 class counts with
        counts_foreground=, as cut_capacities takes them); intensity (B*N) on the 0..255 scale and features (B*N, D) are optional.
        -> (hard labels (B*N,) int64, 1 = foreground; E(S) (B,) float64 = flow / unit; the GraphCut).  Nothing is read back:
        GraphCut.check() reports a graph that did not converge."""
        from .graphcut import cut_capacities, graph_cut
        unit = 1024
        cs, ct, ce = cut_capacities(prior, edge_index, intensity, features, counts_foreground=counts_foreground, gamma=self.gamma_unet_priors,
                                    sigma_intensity=self.sigma_intensity, sigma_features=self.sigma_features, smoothness=smoothness,
                                    unit=unit, batch=batch)
        cut = graph_cut(edge_index, cs, ct, ce, batch=batch)
        return cut.labels.reshape(-1).to(torch.int64), cut.flow.to(torch.float64) / unit, cut

    def solve_multi(self, prior, edge_index, intensity=None, features=None, batch=1, smoothness=1.0):
        """The K-label form of `solve`: alpha-expansion (mgunet.graph_cut_multi) on E(L) = sum_i U_i(L_i) + sum_pairs w_ij [L_i != L_j]
        with the same w_ij.  prior: float32 (B*N, K) class probabilities, or int32 (B*N, K) / (B, N, K) class counts.
        -> (labels (B*N,) int64 in [0, K); E(L) (B,) float64 = energy / unit; the MultiCut).  Nothing is read back: MultiCut.check()
        reports a graph that did not converge."""
        from .graphcut import cut_capacities, graph_cut_multi, label_costs
        unit = 1024
        costs = label_costs(prior, batch=batch, unit=unit)
        half = torch.full((costs.shape[0],), 0.5, dtype=torch.float32, device=costs.device)   # cap_edge does not depend on the prior
        ce = cut_capacities(half, edge_index, intensity, features, gamma=self.gamma_unet_priors, sigma_intensity=self.sigma_intensity,
                            sigma_features=self.sigma_features, smoothness=smoothness, unit=unit, batch=batch)[2]
        cut = graph_cut_multi(edge_index, costs, ce, batch=batch)
        return cut.labels.reshape(-1).to(torch.int64), cut.energy.to(torch.float64) / unit, cut

    def _patch_inputs(self, logits, images_u8, node_features, patch_size):
        """what the two refine_patches feed their solve: (class counts, one image's edge_index, intensity, features, B)"""
        from .patch_graph import PatchGraphConstructor
        from .patch_inputs import patch_labels
        from .preprocess import _to_dev_u8, patch_features_u8
        _lib.require_hip(logits, "mgunet MinCut")
        B, _, H, W = logits.shape
        u8, _ = _to_dev_u8(images_u8)
        if u8.dim() == 3:
            u8 = u8.unsqueeze(0)
        if tuple(u8.shape[:3]) != (B, H, W):
            raise ValueError(f"images_u8 must be ({B}, {H}, {W}, 3) like the logits, got {tuple(u8.shape)}")
        p = int(patch_size)
        graphs = self.__dict__.setdefault("_patch_graphs", {})
        graph = graphs.get(p) or graphs.setdefault(p, PatchGraphConstructor(p))
        _, counts = patch_labels(logits, p, return_counts=True)
        intensity = torch.cat([patch_features_u8(img, p) for img in u8]).reshape(-1)
        feats = node_features.detach().to(torch.float32).reshape(intensity.numel(), -1)
        return counts, graph.edge_index(H, W, logits.device), intensity, feats, B

    def refine_patches_multi(self, logits, images_u8, node_features, patch_size):
        """`refine_patches` over ALL C classes of the U-Net's vote: the label costs come from the per-patch class counts
        (p = (n_k + 1) / (n_all + C)), intensity, features and topology as there.  -> what `solve_multi` returns."""
        counts, ei, intensity, feats, B = self._patch_inputs(logits, images_u8, node_features, patch_size)
        return self.solve_multi(counts, ei, intensity, feats, batch=B)

    def refine_patches(self, logits, images_u8, node_features, patch_size, foreground=1):
        """The patch partition of a batch by the cut, with no trained predictor: the prior is the U-Net's own vote per patch
        (patch_labels(logits, return_counts=True): p = (n_fg + 1) / (n_all + 2) for class `foreground`), the intensity the patch means
        of the uint8 images (patch_features_u8), the features the given node features (B*Np, D) -- the GAT embeddings are the
        intended ones -- and the topology PatchGraphConstructor's.  logits (B, C, H, W) float, images_u8 (B, H, W, 3) uint8.
        -> what `solve` returns."""
        counts, ei, intensity, feats, B = self._patch_inputs(logits, images_u8, node_features, patch_size)
        return self.solve(counts, ei, intensity, feats, batch=B, counts_foreground=int(foreground))

    def compute_edge_weights_for_ncut(self, node_features, edge_index):
        """(E,) weights exp(-|f_i - f_j|^2 / 2) in edge order (:30-52)."""
        _check_features(node_features, "node_features")
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 (2, E) tensor")
        dev = node_features.device
        f = node_features.detach().contiguous()
        ei = edge_index.to(dev).contiguous()
        N, D = f.shape
        E = ei.shape[1]
        if E:
            # the reference raises on an out-of-range index, so this check has to complete before the call returns:
            # ONE reduction and ONE host read (the kernel itself never reads out of range: it trusts this check)
            lo, hi = torch.stack(torch.aminmax(ei)).tolist()
            if lo < 0 or hi >= N:
                raise IndexError(f"edge_index values must be in [0, {N}); got [{lo}, {hi}]")
        w = torch.empty(E, device=dev, dtype=torch.float32)
        _lib.call("mgu_ncut_edge_weights", dev, f, N, D, ei if E else None, E, w if E else None)
        return w

    def _ncut(self, node_features, edge_index, assign, K, is_logits):
        _check_features(node_features, "node_features")
        if torch.is_grad_enabled() and (node_features.requires_grad or assign.requires_grad):
            if node_features.shape[1] > 1024:   # refused here, not in the middle of loss.backward()
                raise ValueError(f"mgu_ncut_backward keeps a feature row in registers: D <= 1024, got {node_features.shape[1]}")
            r = _NcutFn.apply(node_features, assign, self, edge_index, K, is_logits)
            return r if is_logits else (r, None, None)
        return self._ncut_run(node_features, edge_index, assign, K, is_logits)

    def _ncut_run(self, node_features, edge_index, assign, K, is_logits):
        dev = node_features.device
        f = node_features.detach().contiguous()
        N, D = f.shape
        a = assign.detach().to(torch.float32).contiguous()
        rowptr, col = self._csr_by_source(edge_index, N, dev)
        loss = torch.empty(1, device=dev, dtype=torch.float32)
        soft = torch.empty((N, K), device=dev, dtype=torch.float32) if is_logits else None
        hard = torch.empty(N, device=dev, dtype=torch.int32) if is_logits else None
        _lib.call("mgu_ncut_forward", dev, f, N, D, rowptr, col if col.numel() else None, col.numel(), a, K, 1 if is_logits else 0, soft, hard,
                  loss)
        return loss[0], soft, hard

    def forward_batched(self, patch_features, edge_index_single, B, num_expected_segments, segment_logits):
        """The per-image loop of train_end_to_end.py:347-356 for B images that share one patch-graph topology:
        patch_features (B*Np, D), segment_logits (B*Np, K) -> (losses (B,), soft (B*Np, K), hard labels (B*Np,) int64).
        The loss is a quotient per image, so each image is one mgu_ncut_forward call on its slice."""
        N = patch_features.size(0) // B
        losses, softs, hards = [], [], []
        for b in range(B):
            l, s, h = self._ncut(patch_features[b * N:(b + 1) * N], edge_index_single, segment_logits[b * N:(b + 1) * N],
                                 num_expected_segments, True)
            losses.append(l), softs.append(s), hards.append(h)
        return torch.stack(losses), torch.cat(softs, 0), torch.cat(hards, 0).to(torch.int64)

    def normalized_cut_loss(self, node_features, edge_index, segment_assignments_soft, num_segments_k):
        """sum_k cut(A_k, V \\ A_k) / assoc(A_k, V) with soft assignments (:55-160)."""
        N = node_features.size(0)
        if tuple(segment_assignments_soft.shape) != (N, num_segments_k):
            raise ValueError("segment_assignments_soft shape mismatch.")  # :73-74
        return self._ncut(node_features, edge_index, segment_assignments_soft, num_segments_k, False)[0]

    def forward(self, gat_refined_patch_features, patch_graph_edge_index, num_expected_segments, segment_predictor_network=None):
        """(L_partition, soft segment assignments (N, K)): :163-205.  The arg-max labels of train_end_to_end.py:356 come
        out of the same kernel and are kept in `self.last_hard_labels`."""
        if segment_predictor_network is None:
            raise ValueError("segment_predictor_network is required to get segment assignments for Ncut loss.")  # :183-186
        logits = segment_predictor_network(gat_refined_patch_features, patch_graph_edge_index)  # :190
        N = gat_refined_patch_features.size(0)
        if tuple(logits.shape) != (N, num_expected_segments):
            raise ValueError("segment_assignments_soft shape mismatch.")
        loss, soft, hard = self._ncut(gat_refined_patch_features, patch_graph_edge_index, logits, num_expected_segments, True)
        self.last_hard_labels = hard.to(torch.int64)
        return loss, soft
