"""Step loops around the HIP path: replaces the inline loops of
experiments/segmentation_performance.py:119-144 (eval) and scripts/train_end_to_end.py:270-332
(U-Net + patch-graph GAT forward), with the batch sharded over ranks (one process per GPU)."""
from __future__ import annotations

import contextlib
import ctypes as C
import math

import torch
import torch.nn as nn

from . import _lib
from ._args import check_masks, nhwc_storage
from .border import border_options
from .gat import GATNetwork, _csr_cache, _layer_forward, _LayerCall
from .losses import _LOVASZ_CLASSES, pixel_ce_options
from .patch_graph import PatchGraphConstructor
from .unet import UNet

LOSSES = ("ce", "ce+dice", "ce+lovasz", "ce+dice+lovasz")   # what Trainer(loss=...) accepts


class MinGraphUNet(nn.Module):
    """The 'full MinGraph-UNet forward' as one module (the reference has it only as inline code in its
    training loop, train_end_to_end.py:270-332, fed with torch.randn placeholder node features).
    Here: U-Net -> per-patch mean of the shallowest decoder feature -> block-diagonal patch graph of
    the whole batch -> GAT.  Returns (logits, skips, decoder_feats, node_embeddings (B*Np, out_dim))."""

    def __init__(self, unet: UNet, gat: GATNetwork, patch_size: int = 16):
        super().__init__()
        self.unet, self.gat = unet, gat
        self.graph = PatchGraphConstructor(patch_size)

    def forward(self, x):
        B, _, H, W = x.shape
        X = None
        if isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4:
            # ask the U-Net forward to emit the node features (patch means of decoder_feats[0]) in the same pass over
            # the feature map as the final 1x1 conv (mgu_unet_request_patch_mean)
            p = self.graph.patch_size
            X = torch.empty((B * ((H + p - 1) // p) * ((W + p - 1) // p), self.unet.init_features), device=x.device,
                            dtype=torch.float32)
            ctx = self.unet._context(x.device)
            _lib.call("mgu_unet_request_patch_mean", x.device, p, X, ctx=ctx)
        try:
            logits, skips, feats = self.unet(x)
        except Exception:
            if X is not None:   # the forward was rejected before it could serve the request: cancel it
                _lib.call("mgu_unet_request_patch_mean", x.device, 0, None, ctx=ctx)
            raise
        if X is None:
            X = self.graph.patch_mean_features(feats[0])
        rowptr, col, gp, N, E = self.graph.batched_csr(H, W, B, x.device)
        emb = gat_forward_csr(self.gat, X, rowptr, col, gp)
        return logits, skips, feats, emb


class MinGraphUNetE2E(nn.Module):
    """Stages 1-7 of the reference's end-to-end forward (scripts/train_end_to_end.py:270-453) for a whole batch, on
    deterministic node features: U-Net -> patch-mean node features -> patch GAT -> segment predictor +
    normalized-cut loss (mean over images, :425) -> region stage -> FeatureFusion with the shallowest decoder feature ->
    DetectionHead.  Returns a dict with the tensors the loop produces: logits, node embeddings, loss_partition, soft /
    hard patch assignments, region embeddings, fused features, boxes, confidence (and class scores).
    partition="predictor" (default): the hard patch labels are the arg-max of the segment predictor.  partition="mincut"
    (num_segments == 2): they are the exact min cut of MinCutRefinement's energy (MinCutRefinement.refine_patches on the logits, the
    uint8 batch passed as forward(x, images_u8=...) and the node embeddings); the region stage runs on them, soft_assignments /
    loss_partition stay the predictor's, and the dict gains cut_labels (B*Np,) int64 and cut_energy (B,).  partition="expansion"
    (any num_segments >= 2, equal to the U-Net's class count): the same with the K-label cut of
    MinCutRefinement.refine_patches_multi (alpha-expansion over all classes of the U-Net's vote)."""

    def __init__(self, unet: UNet, patch_gat: GATNetwork, segment_predictor, mincut, region_gat: GATNetwork, detection_head,
                 num_segments: int, patch_size: int = 16, partition: str = "predictor", foreground: int = 1):
        super().__init__()
        if partition not in ("predictor", "mincut", "expansion"):
            raise ValueError(f'partition must be "predictor", "mincut" or "expansion", got {partition!r}')
        if partition == "mincut" and num_segments != 2:
            raise ValueError(f'partition="mincut" is a binary cut: num_segments must be 2, got {num_segments}')
        if partition == "expansion" and num_segments < 2:
            raise ValueError(f'partition="expansion" needs num_segments >= 2, got {num_segments}')
        self.partition, self.foreground = partition, foreground
        self.core = MinGraphUNet(unet, patch_gat, patch_size)
        self.segment_predictor, self.mincut, self.region_gat, self.detection_head = segment_predictor, mincut, region_gat, detection_head
        self.num_segments = num_segments

    @torch.no_grad()   # a pipeline of forward values (the pooling / cut / fuse kernels between the modules carry no autograd graph)
    def forward(self, x, images_u8=None):
        from .region import region_stage
        B, _, H, W = x.shape
        if self.partition != "predictor" and images_u8 is None:
            raise ValueError(f'partition="{self.partition}" needs the uint8 batch: forward(x, images_u8=...)')
        logits, skips, feats, emb = self.core(x)
        if self.partition == "expansion" and logits.shape[1] != self.num_segments:
            raise ValueError(f'partition="expansion" labels the patches with the U-Net\'s classes: the logits have {logits.shape[1]} classes, '
                             f"num_segments is {self.num_segments}")
        graph = self.core.graph
        nph, npw = graph.grid(H, W)
        K = self.num_segments
        ei_one = graph.edge_index(H, W, x.device)                                   # one image's COO (all images share it)
        if getattr(self.segment_predictor, "use_gnn", False):
            ei_all = graph.edge_index(H, W, x.device, B)
            gp = graph.batched_csr(H, W, B, x.device)[2]                            # per-graph max e (graph_attention.py:86)
            seg_logits = self.segment_predictor.gnn_predictor(emb, ei_all, graph_ptr=gp)
        else:
            seg_logits = self.segment_predictor(emb)
        losses, soft, hard = self.mincut.forward_batched(emb, ei_one, B, K, seg_logits.contiguous())
        cut = None
        if self.partition == "mincut":
            cut = self.mincut.refine_patches(logits, images_u8, emb, graph.patch_size, self.foreground)
            hard = cut[0]
        elif self.partition == "expansion":
            cut = self.mincut.refine_patches_multi(logits, images_u8, emb, graph.patch_size)
            hard = cut[0]
        region_emb, fused = region_stage(emb, hard, B, K, self.region_gat, nph, npw, H, W, f_u=feats[0])
        det = self.detection_head(fused)
        out = {"logits": logits, "skips": skips, "decoder_feats": feats, "node_embeddings": emb, "loss_partition": losses.mean(),
               "soft_assignments": soft, "hard_labels": hard, "region_embeddings": region_emb, "fused": fused,
               "bboxes": det[0], "confidence": det[1]}
        if len(det) > 2:
            out["class_scores"] = det[2]
        if cut is not None:
            out["cut_labels"], out["cut_energy"] = cut[0], cut[1]
        return out


def gat_forward_csr(gat: GATNetwork, X, rowptr, col, graph_ptr):
    """GATNetwork.forward in eval mode on a prebuilt device CSR (skips the COO->CSR conversion of the COO API; no autograd node)."""
    h = X
    for layer in gat.gat_layers:
        if layer.training and layer.dropout_rate > 0:
            raise RuntimeError("gat_forward_csr is the inference schedule on a prebuilt CSR: call .eval(), or run the layer through "
                               "GATNetwork.forward(X, edge_index) for train-mode dropout (see mgunet.gat)")
        heads = list(layer.heads)
        if heads[0].W.weight.shape[1] != h.shape[1]:
            raise ValueError("node feature width must match W")
        h = _layer_forward(_LayerCall(heads, h, layer.concat, layer.alpha, _csr_cache(layer), graph_ptr, csr=(rowptr, col)), None)
    return h


def argmax_classes(logits_nchw: torch.Tensor) -> torch.Tensor:
    """torch.argmax(seg_logits, dim=1) of segmentation_performance.py:141 on the GPU (NHWC logits)."""
    _lib.require_hip(logits_nchw, "argmax_classes")
    B, Cc, H, W = logits_nchw.shape
    nhwc = nhwc_storage(logits_nchw)
    pred = torch.empty((B, H, W), device=logits_nchw.device, dtype=torch.int64)
    _lib.call("mgu_argmax_classes", logits_nchw.device, nhwc, B * H * W, Cc, pred)
    return pred


@torch.no_grad()
def segment_batch(model: UNet, images: torch.Tensor):
    """One iteration of the eval loop (segmentation_performance.py:125-141): logits, argmax mask."""
    logits, _, _ = model(images)
    return logits, argmax_classes(logits)


def shard_batch(global_batch: int, rank: int, world_size: int):
    """Contiguous image range [lo, hi) of this rank: images (and their graphs) are independent in
    forward, so inference shards with no collective."""
    base, rem = divmod(global_batch, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def allreduce_mean_(flat: torch.Tensor, group=None) -> float:
    """Sum-all-reduce `flat` in place over the ranks (RCCL over xGMI when the backend is "nccl") and return
    the factor (1/world) that turns the sum into the mean; 1.0 and no collective for a single process.
    One flat pre-packed buffer = one collective per step (31 MB for UNet(3,2,32,4))."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1.0
    world = dist.get_world_size(group)
    if world == 1:
        return 1.0
    if flat.is_cuda and dist.get_backend(group) == "gloo":   # rehearsal only: gloo has no device path here
        host = flat.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        flat.copy_(host)
    else:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    return 1.0 / world


def adam_state_dict(params, exp_avg_flat, exp_avg_sq_flat, step, lr, betas, eps, weight_decay, decoupled=False) -> dict:
    """torch.optim.Adam.state_dict() layout from flat moment buffers in named_parameters() order (pure tensor plumbing: runs on any
    device; the CPU tier checks it against a real torch.optim.Adam).  decoupled: torch.optim.AdamW's layout, the same with
    decoupled_weight_decay set."""
    state, off = {}, 0
    for i, p in enumerate(params):
        k = p.numel()
        if step > 0:
            state[i] = {"step": torch.tensor(float(step)), "exp_avg": exp_avg_flat[off:off + k].detach().clone().view_as(p),
                        "exp_avg_sq": exp_avg_sq_flat[off:off + k].detach().clone().view_as(p)}
        off += k
    group = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": weight_decay, "amsgrad": False, "maximize": False, "foreach": None,
             "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": bool(decoupled), "params": list(range(len(params)))}
    return {"state": state, "param_groups": [group]}


class StepLR:
    """optim.lr_scheduler.StepLR(optimizer, step_size, gamma) for a Trainer (train_segmentation.py:105, stepped once per epoch at
    :143): lr = base_lr * gamma ** (epoch // step_size)."""

    def __init__(self, trainer, step_size: int, gamma: float = 0.1):
        self.trainer, self.step_size, self.gamma = trainer, int(step_size), float(gamma)
        self.base_lr, self.last_epoch = trainer.lr, 0

    def step(self) -> None:
        self.last_epoch += 1
        self.trainer.set_lr(self.base_lr * self.gamma ** (self.last_epoch // self.step_size))

    def get_last_lr(self):
        return [self.trainer.lr]

    def state_dict(self) -> dict:
        return {"step_size": self.step_size, "gamma": self.gamma, "base_lrs": [self.base_lr], "last_epoch": self.last_epoch}

    def load_state_dict(self, sd: dict) -> None:
        self.step_size, self.gamma, self.base_lr, self.last_epoch = sd["step_size"], sd["gamma"], sd["base_lrs"][0], sd["last_epoch"]
        self.trainer.set_lr(self.base_lr * self.gamma ** (self.last_epoch // self.step_size))


class CosineAnnealingLR:
    """optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max, eta_min) for a Trainer, stepped once per epoch: torch's own
    recurrence on the current learning rate (not the closed form, which differs from it in the last bits), so the sequence equals
    torch's with ==."""

    def __init__(self, trainer, T_max: int, eta_min: float = 0.0):
        self.trainer, self.T_max, self.eta_min = trainer, int(T_max), float(eta_min)
        self.base_lr, self.last_epoch = trainer.lr, 0

    def step(self) -> None:
        m, T, lr = math, self.T_max, self.trainer.lr
        self.last_epoch += 1
        if (self.last_epoch - 1 - T) % (2 * T) == 0:
            lr = lr + (self.base_lr - self.eta_min) * (1 - m.cos(m.pi / T)) / 2
        else:
            lr = (1 + m.cos(m.pi * self.last_epoch / T)) / (1 + m.cos(m.pi * (self.last_epoch - 1) / T)) * (lr - self.eta_min) + self.eta_min
        self.trainer.set_lr(lr)

    def get_last_lr(self):
        return [self.trainer.lr]

    def state_dict(self) -> dict:
        return {"T_max": self.T_max, "eta_min": self.eta_min, "base_lrs": [self.base_lr], "last_epoch": self.last_epoch,
                "_last_lr": [self.trainer.lr]}

    def load_state_dict(self, sd: dict) -> None:
        self.T_max, self.eta_min, self.base_lr, self.last_epoch = sd["T_max"], sd["eta_min"], sd["base_lrs"][0], sd["last_epoch"]
        self.trainer.set_lr(sd["_last_lr"][0])     # the recurrence continues from the rate it had reached


class ReduceLROnPlateau:
    """optim.lr_scheduler.ReduceLROnPlateau for a Trainer: step(metric) once per epoch; after more than `patience` epochs without
    an improvement (by `threshold`, relative or absolute) the rate becomes max(lr * factor, min_lr) where that lowers it by more than
    `eps`, and `cooldown` epochs pass before bad epochs count again.  torch's own comparisons in torch's order."""

    def __init__(self, trainer, mode="min", factor=0.1, patience=10, threshold=1e-4, threshold_mode="rel", cooldown=0, min_lr=0.0,
                 eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if mode not in ("min", "max"):
            raise ValueError(f"mode {mode} is unknown!")
        if threshold_mode not in ("rel", "abs"):
            raise ValueError(f"threshold mode {threshold_mode} is unknown!")
        self.trainer, self.mode, self.factor, self.patience = trainer, mode, float(factor), int(patience)
        self.threshold, self.threshold_mode, self.cooldown, self.min_lr, self.eps = threshold, threshold_mode, int(cooldown), float(min_lr), eps
        self.best = float("inf") if mode == "min" else -float("inf")
        self.cooldown_counter, self.num_bad_epochs, self.last_epoch = 0, 0, 0

    def _is_better(self, a, best) -> bool:
        if self.mode == "min" and self.threshold_mode == "rel":
            return a < best * (1.0 - self.threshold)
        if self.mode == "min":
            return a < best - self.threshold
        if self.threshold_mode == "rel":
            return a > best * (self.threshold + 1.0)
        return a > best + self.threshold

    def step(self, metrics) -> None:
        current = float(metrics)
        self.last_epoch += 1
        if self._is_better(current, self.best):
            self.best, self.num_bad_epochs = current, 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            old = float(self.trainer.lr)
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.trainer.set_lr(new)
            self.cooldown_counter, self.num_bad_epochs = self.cooldown, 0

    def get_last_lr(self):
        return [self.trainer.lr]

    _KEYS = ("mode", "factor", "patience", "threshold", "threshold_mode", "cooldown", "min_lr", "eps", "best", "cooldown_counter",
             "num_bad_epochs", "last_epoch")

    def state_dict(self) -> dict:
        return {**{k: getattr(self, k) for k in self._KEYS}, "_last_lr": [self.trainer.lr]}

    def load_state_dict(self, sd: dict) -> None:
        for k in self._KEYS:
            setattr(self, k, sd[k])
        self.trainer.set_lr(sd["_last_lr"][0])


class _DeviceStep:
    """What Trainer and FlatAdam share of the optimizer step whose decisions stay on the device (mgu_optim_step, INTEGRATION.md
    section X): the options, the 64-byte control record, the EMA buffer.  The host class has flat / grad / exp_avg / exp_avg_sq,
    lr / wd / betas / eps / momentum and device."""

    def _init_device_step(self, kind, max_grad_norm, skip_nonfinite, ema_decay, ema_warmup, always=False) -> None:
        self.optim_kind = kind
        self.max_grad_norm, self.skip_nonfinite = float(max_grad_norm), bool(skip_nonfinite)
        self.ema_decay, self.ema_warmup = float(ema_decay), bool(ema_warmup)
        # with every option at its default and Adam or SGD the step stays the one mgu_adam_step / mgu_sgd_step launch
        self.device_step = bool(always or kind == "adamw" or self.max_grad_norm > 0.0 or self.skip_nonfinite or self.ema_decay > 0.0)
        self.ctrl = self.ema = None

    @staticmethod
    def _check_step_options(max_grad_norm, ema_decay) -> None:
        if not (float(max_grad_norm) >= 0.0 and float(max_grad_norm) != float("inf")):
            raise ValueError(f"max_grad_norm must be finite and >= 0 (0: no clipping), got {max_grad_norm}")
        if not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must lie in [0, 1) (0: no EMA), got {ema_decay}")

    def _alloc_device_step(self) -> None:
        """After the flat buffer holds the parameters: the zeroed record (a fresh optimizer) and the EMA as a copy of them."""
        if self.device_step:
            self.ctrl = torch.zeros(_lib.OPTIM_CTRL_BYTES // 8, device=self.device, dtype=torch.int64)
        if self.ema_decay > 0.0:
            self.ema = self.flat.detach().clone()

    def _device_optim_step(self, grad, grad_scale, ctx=None) -> None:
        d = _lib.OptimDesc(_lib.OPTIM_KINDS[self.optim_kind], self.lr, self.betas[0], self.betas[1], self.eps, self.wd,
                           getattr(self, "momentum", 0.0), grad_scale, self.max_grad_norm, int(self.skip_nonfinite), self.ema_decay,
                           int(self.ema_warmup))
        _lib.call("mgu_optim_step", self.device, C.byref(d), self.flat, grad, self.exp_avg,
                  None if self.optim_kind == "sgd" else self.exp_avg_sq, self.ema, self.ctrl, self.flat.numel(), ctx=ctx)

    def _need_record(self) -> None:
        if self.ctrl is None:
            raise RuntimeError("this optimizer steps through mgu_adam_step / mgu_sgd_step and keeps no control record: it has one with "
                               "optimizer='adamw', max_grad_norm, skip_nonfinite or ema_decay")

    @property
    def grad_norm(self) -> torch.Tensor:
        """L2 norm of the last step's scaled gradient (before clipping): a float64 device scalar, a view of the record -- reading it
        here does not synchronise."""
        self._need_record()
        return self.ctrl.view(torch.float64)[3]

    def applied_steps(self) -> int:
        """Steps the device applied (the record's `step`).  Synchronises."""
        self._need_record()
        return int(self.ctrl[0])

    def skipped_steps(self) -> int:
        """Steps skipped for a non-finite gradient (the record's `skipped`).  Synchronises."""
        self._need_record()
        return int(self.ctrl[1])

    def _set_device_steps(self, step: int) -> None:
        if self.ctrl is not None:
            self.ctrl[0] = int(step)


class Trainer(_DeviceStep):
    """The train step of scripts/train_segmentation.py:117-137 on the HIP path:
    zero_grad -> logits = model(images) (train-mode BatchNorm) -> CrossEntropyLoss (mean) -> backward ->
    [mean all-reduce of the flat gradient over the data-parallel ranks] -> Adam(lr, weight_decay as L2).
    Parameters are re-homed as views of ONE flat fp32 buffer (named_parameters() order) so the optimizer is
    a single kernel and the gradient exchange a single collective.  Each rank normalises BatchNorm over its
    own shard (DDP semantics)."""

    def __init__(self, model: UNet, lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, process_group=None, comm="auto",
                 loss="ce", dice_smooth=1.0, optimizer="adam", momentum=0.9, lovasz_per_image=False, lovasz_classes="present",
                 ce_weight=None, label_smoothing=0.0, focal_gamma=0.0, hard_fraction=1.0, hard_min_kept=0, hard_per_image=False,
                 border_w0=0.0, border_sigma=5.0, border_connectivity=2, border_separate=False, max_grad_norm=0.0,
                 skip_nonfinite=False, ema_decay=0.0, ema_warmup=False, accumulate=1):
        """comm: "auto" (default) -- with more than one rank the gradient is mean-all-reduced by torch.distributed (RCCL when the
        backend is "nccl") after backward: the path exercised with two ranks.  "rccl" -- opt in to libmgunet's own RCCL
        communicator with the bucketed exchange overlapped with backward (mgu_unet_backward_allreduce); tests/test_gpu_rccl.py
        runs it with two ranks on a box that has two GPUs and with one rank elsewhere.  None -- no exchange.
        loss: "ce" -- nn.CrossEntropyLoss() alone (train_segmentation.py:91,127); "ce+dice" -- the sum the script forms at
        :126-130, `criterion_ce(logits, masks) + dice_loss(logits, masks)`: the Dice gradient (through the softmax) is added to
        the cross-entropy gradient in the same dlogits buffer (mgu_dice_loss_backward, accumulate) before the one backward pass.
        "ce+lovasz" / "ce+dice+lovasz" -- additionally the Lovasz-Softmax loss (losses.lovasz_softmax, the IoU surrogate; options
        lovasz_per_image, lovasz_classes), added the same way after them: one mgu_lovasz_softmax_backward(accumulate) call.
        ce_weight, label_smoothing, focal_gamma, hard_fraction, hard_min_kept, hard_per_image: the options of
        losses.pixel_cross_entropy (weight, label_smoothing, focal_gamma, keep_fraction, min_kept, per_image; INTEGRATION.md section
        S).  With all six at their defaults the cross-entropy term is mgu_cross_entropy, exactly as before; otherwise one
        mgu_pixel_ce_backward call takes its place and the dice / Lovasz terms accumulate after it as they do after the plain one.
        border_w0, border_sigma, border_connectivity, border_separate: the U-Net paper's border weight map (mgunet.border_weights,
        INTEGRATION.md section V).  With border_w0 > 0 every step labels its masks (the `instances` given to train_step, else
        mgu_connected_components of the class masks with border_connectivity, foreground = not class 0), forms the map
        ce_weight[class] + border_w0 exp(-(d1 + d2)^2 / (2 border_sigma^2)) on the device and hands it to mgu_pixel_ce_map_backward,
        which takes the cross-entropy call's place (the class weights are then in the map, not in the loss a second time);
        border_separate also trains on the target with touching instances set one pixel apart.  With border_w0 == 0, the default,
        the step launches nothing new and calls exactly what it called before.
        ("rccl" also creates the communicator for a single process: the collective then degenerates to a copy.)
        optimizer: "adam" (train_segmentation.py:96, the shipped configs/training.yaml) or "sgd" -- the script's other branch,
        optim.SGD(lr, momentum=sgd_momentum, weight_decay) (:97-98; training.yaml:5-6): one fused kernel on the flat buffers either way;
        or "adamw", torch.optim.AdamW (decoupled weight decay).
        max_grad_norm, skip_nonfinite, ema_decay, ema_warmup, accumulate: with all five at their defaults
        and "adam" or "sgd" the step is the one mgu_adam_step / mgu_sgd_step call it has always been.  Otherwise it is one
        mgu_optim_step -- three launches, every decision on the device, the host never blocked: max_grad_norm > 0 clips the averaged,
        scaled gradient to that L2 norm (torch.nn.utils.clip_grad_norm_'s arithmetic on a norm summed in double in a fixed order;
        `grad_norm` is the device scalar); skip_nonfinite leaves parameters, moments, EMA and the step count of the bias corrections
        untouched when the gradient holds an inf or a NaN (`skipped_steps()`); ema_decay > 0 keeps an exponential moving average of the
        parameters, a copy of them at the start (ema_warmup: decay min(ema_decay, (1 + t) / (10 + t)) at step t; `ema_state_dict()`,
        `with trainer.ema_weights():`).  accumulate=k: train_step runs forward and backward every call and adds the gradient into an
        accumulator (mgu_grad_accumulate); the k-th call exchanges the accumulator (comm="auto": one all-reduce) and steps with
        grad_scale = 1 / (k * world).  comm="rccl" with accumulate > 1 raises ValueError: that exchange runs inside backward, bucket
        by bucket on each call's gradient, and has no accumulator to work on."""
        if optimizer not in _lib.OPTIM_KINDS:
            raise ValueError(f"unknown optimizer {optimizer!r}: 'adam', 'adamw' or 'sgd'")
        self._check_step_options(max_grad_norm, ema_decay)
        if int(accumulate) != accumulate or accumulate < 1:
            raise ValueError(f"accumulate must be an integer >= 1, got {accumulate}")
        if comm == "rccl" and accumulate > 1:
            raise ValueError('comm="rccl" exchanges each backward\'s gradient inside that backward: it cannot be combined with accumulate > 1 '
                             '(use comm="auto")')
        if loss not in LOSSES:
            raise ValueError(f"unknown loss {loss!r}: " + ", ".join(repr(k) for k in LOSSES[:-1]) + f" or {LOSSES[-1]!r}")
        if lovasz_classes not in _LOVASZ_CLASSES:
            raise ValueError(f"unknown lovasz_classes {lovasz_classes!r}: 'present' or 'all'")
        pixel_ce = pixel_ce_options(ce_weight, label_smoothing, focal_gamma, hard_fraction, hard_min_kept, hard_per_image, getattr(model, "num_classes", None))
        if border_connectivity not in (1, 2):
            raise ValueError(f"border_connectivity must be 1 (4-neighbours) or 2 (8-neighbours), got {border_connectivity}")
        w0, sigma = border_options(border_w0, border_sigma)
        if w0 > 0.0:
            border_options(w0, sigma, getattr(model, "num_classes", None), ce_weight)
        self.optimizer, self.momentum = optimizer, float(momentum)
        params = list(model.named_parameters())
        _lib.require_hip(params[0][1], "Trainer")
        self.model, self.group = model, process_group
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        dev = params[0][1].device
        self.device = dev
        ctx = model._context(dev)
        n = int(_lib.lib().mgu_unet_param_count(ctx.handle))
        if n != sum(p.numel() for _, p in params):
            raise RuntimeError("parameter count mismatch between the module tree and libmgunet")
        self.flat = torch.empty(n, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(n, device=dev, dtype=torch.float32)
        self.exp_avg = torch.zeros(n, device=dev, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(n, device=dev, dtype=torch.float32)
        off = 0
        for name, p in params:  # named_parameters() order must be the library's flat order
            lo = int(_lib.lib().mgu_unet_param_offset(ctx.handle, name.encode()))
            if lo != off:
                raise RuntimeError(f"flat parameter layout mismatch at {name}: {lo} != {off}")
            k = p.numel()
            self.flat[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.flat[off:off + k].view_as(p)
            p.grad = self.grad[off:off + k].view_as(p)
            off += k
        model.mark_parameters_changed()
        model._slots = None
        self.step_count = 0
        self.accumulate, self._micro = int(accumulate), 0
        self.acc = torch.zeros(n, device=dev, dtype=torch.float32) if self.accumulate > 1 else None
        self._init_device_step(optimizer, max_grad_norm, skip_nonfinite, ema_decay, ema_warmup, always=self.accumulate > 1)
        self._alloc_device_step()
        self.loss_kind, self.dice_smooth = loss, float(dice_smooth)
        self.lovasz_mode, self.lovasz_per_image = _LOVASZ_CLASSES[lovasz_classes], int(bool(lovasz_per_image))
        self._lovasz = torch.zeros(1, device=dev, dtype=torch.float32)
        # the pixel cross-entropy's options, None while all of them are at their defaults (the step then calls mgu_cross_entropy)
        self.pixel_ce = None if ce_weight is None and pixel_ce == (0.0, 0.0, 1.0, 0, 0) else pixel_ce
        self.ce_weight = None if ce_weight is None else ce_weight.detach().to(device=dev, dtype=torch.float32).contiguous()
        # the border weight map's options, None while border_w0 == 0 (the step then forms no map)
        self.border = None if w0 == 0.0 else (w0, sigma, int(border_connectivity), bool(border_separate))
        self._loss = torch.zeros(1, device=dev, dtype=torch.float32)
        self._dice = torch.zeros(1, device=dev, dtype=torch.float32)
        self._rccl = False
        if comm not in ("auto", "rccl", None):
            raise ValueError(f"unknown comm {comm!r}: 'auto', 'rccl' or None")
        self.comm = comm
        if comm == "rccl":
            self.attach_rccl()

    def _dist_world(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def _dist_backend(self):
        import torch.distributed as dist
        return dist.get_backend(self.group) if dist.is_available() and dist.is_initialized() else None

    def attach_rccl(self) -> None:
        """ncclCommInitRank inside libmgunet for this rank's context.  Rank 0 draws the ncclUniqueId; the launcher's process
        group is used ONLY to hand its 128 bytes to the other ranks."""
        import torch.distributed as dist
        ctx = self.model._context(self.device)
        world, rank = self._dist_world(), (dist.get_rank(self.group) if self._dist_world() > 1 else 0)
        buf = C.create_string_buffer(128)
        if rank == 0:
            _lib.call("mgu_comm_get_unique_id", None, buf)
        if world > 1:
            box = [bytes(buf.raw)]
            with torch.cuda.device(self.device):   # an NCCL group moves the pickled object through the CURRENT device
                dist.broadcast_object_list(box, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)
            buf = C.create_string_buffer(box[0], 128)
        _lib.call("mgu_comm_init_rank", self.device, buf, rank, world, ctx=ctx)
        self._rccl = True

    def set_lr(self, lr: float) -> None:  # schedulers live on the host (train_segmentation.py:105,143): see StepLR below
        self.lr = lr

    # ---- torch.optim.Adam-compatible optimizer state (train_segmentation.py:154-164 saves optimizer.state_dict()) ------------
    def optimizer_state_dict(self) -> dict:
        """What torch.optim.Adam(model.parameters(), lr, weight_decay=wd).state_dict() would hold after the same steps: per
        parameter {'step', 'exp_avg', 'exp_avg_sq'} (views of the flat moment buffers, cloned) + one param_group.  Loadable into a
        real torch.optim.Adam, and back (load_optimizer_state_dict).  optimizer="adamw": the layout of torch.optim.AdamW, loadable
        into a real one.  With skip_nonfinite the step count is the record's (a skipped step does not count): that read synchronises."""
        steps = self.applied_steps() if self.skip_nonfinite else self.step_count
        if self.optimizer == "sgd":   # torch.optim.SGD's layout: {'momentum_buffer'} per parameter, one param_group
            params = [p for _, p in self.model.named_parameters()]
            state, off = {}, 0
            for i, p in enumerate(params):
                k = p.numel()
                if steps > 0 and self.momentum != 0:
                    state[i] = {"momentum_buffer": self.exp_avg[off:off + k].view_as(p).clone()}
                off += k
            return {"state": state, "param_groups": [{"lr": self.lr, "momentum": self.momentum, "dampening": 0, "weight_decay": self.wd,
                                                      "nesterov": False, "maximize": False, "foreach": None, "differentiable": False,
                                                      "fused": None, "params": list(range(len(params)))}]}
        return adam_state_dict([p for _, p in self.model.named_parameters()], self.exp_avg, self.exp_avg_sq, steps,
                               self.lr, self.betas, self.eps, self.wd, decoupled=self.optimizer == "adamw")

    def load_optimizer_state_dict(self, sd: dict) -> None:
        params = [p for _, p in self.model.named_parameters()]
        g = sd["param_groups"][0]
        if self.optimizer == "sgd":
            if len(sd["param_groups"]) != 1 or list(g["params"]) != list(range(len(params))):
                raise ValueError("expected the single param_group of optim.SGD(model.parameters(), ...) (train_segmentation.py:98)")
            self.lr, self.momentum, self.wd = float(g["lr"]), float(g["momentum"]), float(g["weight_decay"])
            off, have = 0, 0
            for i, p in enumerate(params):
                k = p.numel()
                st = sd["state"].get(i)
                if st is not None and st.get("momentum_buffer") is not None:
                    self.exp_avg[off:off + k].copy_(st["momentum_buffer"].reshape(-1))
                    have += 1
                off += k
            if have not in (0, len(params)):
                raise ValueError("a momentum buffer for some parameters only cannot be represented by the fused flat SGD")
            self.step_count = 2 if have else 0     # SGD keeps no step count: any value past the first step continues the buffers
            self._set_device_steps(self.step_count)
            return
        if len(sd["param_groups"]) != 1 or list(g["params"]) != list(range(len(params))):
            raise ValueError("expected the single param_group of optim.Adam(model.parameters(), ...) (train_segmentation.py:96)")
        self.lr, self.betas, self.eps, self.wd = float(g["lr"]), tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"])
        off, steps = 0, set()
        for i, p in enumerate(params):
            k = p.numel()
            st = sd["state"].get(i)
            if st is None:                                    # a parameter Adam has not stepped yet
                self.exp_avg[off:off + k].zero_()
                self.exp_avg_sq[off:off + k].zero_()
            else:
                self.exp_avg[off:off + k].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
                steps.add(int(st["step"]))
            off += k
        if len(steps) > 1:
            raise ValueError("parameters with different step counts cannot be represented by the fused flat Adam")
        self.step_count = steps.pop() if steps else 0
        self._set_device_steps(self.step_count)

    # ---- the averaged weights (ema_decay > 0) -------------------------------------------------------------------------------------
    def _need_ema(self) -> None:
        if self.ema is None:
            raise RuntimeError("this Trainer keeps no EMA of its parameters: construct it with ema_decay > 0")

    def ema_state_dict(self) -> dict:
        """The model's state_dict with every parameter replaced by its moving average; the buffers (BatchNorm running statistics)
        are the live model's: they are not averaged."""
        self._need_ema()
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        off = 0
        for name, p in self.model.named_parameters():
            k = p.numel()
            sd[name] = self.ema[off:off + k].view_as(p).clone()
            off += k
        return sd

    def load_ema_state_dict(self, sd: dict) -> None:
        self._need_ema()
        off = 0
        for name, p in self.model.named_parameters():
            k = p.numel()
            self.ema[off:off + k].copy_(sd[name].reshape(-1))
            off += k

    def _swap_ema(self) -> None:
        live = self.flat.clone()
        self.flat.copy_(self.ema)
        self.ema.copy_(live)
        self.model.mark_parameters_changed()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the model runs on the averaged parameters: the flat buffer and the EMA buffer change places on the
        device (three copies, the parameters stay views of the flat buffer) and the model is told its parameters changed; on exit
        they change back, bit for bit, and training continues.  Do not step inside the block."""
        self._need_ema()
        self._swap_ema()
        try:
            yield self.model
        finally:
            self._swap_ema()

    def save_checkpoint(self, path: str, epoch: int, loss: float) -> None:
        """The reference's checkpoint dict (train_segmentation.py:158-163): readable by its own loaders
        (infer_segmentation.py:90-95, segmentation_performance.py:86-110) and by torch.optim.Adam.  With ema_decay > 0 it carries one more key, "ema_state_dict" (ema_state_dict()); those loaders
        read the keys they know and ignore it."""
        ck = {"epoch": epoch, "model_state_dict": {k: v.detach().clone() for k, v in self.model.state_dict().items()},
              "optimizer_state_dict": self.optimizer_state_dict(), "loss": loss}
        if self.ema is not None:
            ck["ema_state_dict"] = self.ema_state_dict()
        torch.save(ck, path)

    def load_checkpoint(self, path: str) -> dict:
        """Resume from either layout the reference writes: the checkpoint dict or a bare state_dict (:166-168).  Returns the dict."""
        ck = torch.load(path, map_location=self.device)
        sd = ck["model_state_dict"] if isinstance(ck, dict) and "model_state_dict" in ck else ck
        with torch.no_grad():
            own = dict(self.model.state_dict())
            for k, v in sd.items():
                own[k].copy_(v)                               # in place: parameters stay views of the flat buffer
        self.model.mark_parameters_changed()
        if isinstance(ck, dict) and "optimizer_state_dict" in ck:
            self.load_optimizer_state_dict(ck["optimizer_state_dict"])
        if self.ema is not None:      # a checkpoint written without EMA restarts the average from the loaded parameters
            if isinstance(ck, dict) and "ema_state_dict" in ck:
                self.load_ema_state_dict(ck["ema_state_dict"])
            else:
                self.ema.copy_(self.flat)
        return ck if isinstance(ck, dict) else {"model_state_dict": ck}

    def _border_map(self, masks: torch.Tensor, instances, num_classes: int, ctx):
        """(weight map fp32 (B, H, W), the target the cross-entropy trains on) of this step's masks: mgu_border_weights' two launches
        on `instances`, or on the labels mgu_connected_components makes of the masks first; no host synchronisation."""
        w0, sigma, connectivity, separate = self.border
        B, H, W = masks.shape
        dev = self.device
        if instances is None:
            lab = torch.empty((B, H, W), device=dev, dtype=torch.int32)
            _lib.call("mgu_connected_components", dev, masks, 0, B, H, W, 0, connectivity, 0, int(num_classes), 0, lab,
                      torch.empty(B, device=dev, dtype=torch.int64), torch.empty(B + 1, device=dev, dtype=torch.int64), ctx=ctx)
        else:
            if not isinstance(instances, torch.Tensor) or instances.is_floating_point() or not instances.is_cuda:
                raise TypeError("instances must be an integer tensor on the HIP device")
            check_masks(instances, B, H, W)
            lab = instances.to(torch.int32).contiguous()
        weight = torch.empty((B, H, W), device=dev, dtype=torch.float32)
        target = torch.empty((B, H, W), device=dev, dtype=torch.int64) if separate else None
        _lib.call("mgu_border_weights", dev, lab, B, H, W, masks, self.ce_weight, 0 if self.ce_weight is None else self.ce_weight.numel(),
                  w0, sigma, 0, None, None, None, weight, target, ctx=ctx)
        return weight, (target if separate else masks)

    def forward_backward(self, images: torch.Tensor, masks: torch.Tensor, exchange: bool = False, instances=None) -> torch.Tensor:
        """Fills self.grad with d(mean CE)/d(params) of this rank's shard; returns the loss (device scalar).
        exchange=True (needs attach_rccl): the gradient comes back already averaged over the ranks, the all-reduce having run
        bucket by bucket behind the layers still being differentiated.  instances: with border_w0 > 0, the int (B, H, W) instance
        map of the masks (0 = background) in the place of their connected components."""
        model, dev = self.model, self.device
        if masks.dtype != torch.int64 or not masks.is_cuda:
            raise TypeError("masks must be an int64 tensor on the HIP device")
        model.train()
        logits, _, _ = model(images)
        B, Cc, H, W = logits.shape
        check_masks(masks, B, H, W)
        ctx = model._context(dev)
        nhwc = nhwc_storage(logits)   # the forward's own storage: no copy
        masks = masks.contiguous()
        npix = B * H * W
        ldd = (Cc + 3) // 4 * 4
        dlogits = torch.empty((npix, ldd), device=dev, dtype=torch.float32)
        loss = self._loss
        if self.border is not None:   # the class weights are the map's class term: the loss takes the map alone
            pmap, target = self._border_map(masks, instances, Cc, ctx)
            _lib.call("mgu_pixel_ce_map_backward", dev, nhwc, target, B, H * W, Cc, H * W * Cc, 1, Cc, None, pmap,
                      *(self.pixel_ce or (0.0, 0.0, 1.0, 0, 0)), -100, 1.0, None, dlogits, H * W * ldd, 1, ldd, 0, ldd, self._loss, ctx=ctx)
        elif self.pixel_ce is None:
            _lib.call("mgu_cross_entropy", dev, nhwc, masks, npix, Cc, 1.0 / npix, dlogits, self._loss, ctx=ctx)
        else:   # weights, smoothing, the focal term or hard-pixel mining: the same rows of dlogits, padding classes zeroed
            _lib.call("mgu_pixel_ce_backward", dev, nhwc, masks, B, H * W, Cc, H * W * Cc, 1, Cc, self.ce_weight, *self.pixel_ce, -100,
                      1.0, None, dlogits, H * W * ldd, 1, ldd, 0, ldd, self._loss, ctx=ctx)
        if "dice" in self.loss_kind:   # loss = loss_ce + loss_dice (:130): d(dice)/d(logits) is ADDED to the CE gradient
            _lib.call("mgu_dice_loss_backward", dev, nhwc, masks, B, H * W, Cc, H * W * Cc, 1, Cc, self.dice_smooth, 1.0, None, dlogits,
                      H * W * ldd, 1, ldd, 1, self._dice, ctx=ctx)
            loss = self._loss + self._dice
        if "lovasz" in self.loss_kind:   # ... and so is d(lovasz)/d(logits)
            _lib.call("mgu_lovasz_softmax_backward", dev, nhwc, masks, B, H * W, Cc, H * W * Cc, 1, Cc, self.lovasz_mode,
                      self.lovasz_per_image, -100, 1.0, None, dlogits, H * W * ldd, 1, ldd, 1, self._lovasz, ctx=ctx)
            loss = loss + self._lovasz
        _lib.call("mgu_unet_backward_allreduce" if exchange else "mgu_unet_backward", dev, dlogits, self.grad, ctx=ctx)
        return loss

    def check(self) -> None:
        """Synchronise and raise ValueError if a kernel of this trainer met invalid data (a label outside [0, C) other than
        the ignore_index -100) -- the place torch would have raised; train_step itself never blocks the host."""
        _lib.call("mgu_sync_check", self.device, ctx=self.model._context(self.device))

    def optimizer_step(self, grad_scale: float = 1.0, grad=None) -> None:
        """One step on `grad` (default: self.grad, what forward_backward filled) scaled by grad_scale."""
        model, dev = self.model, self.device
        ctx = model._context(dev)
        grad = self.grad if grad is None else grad
        self.step_count += 1
        if self.device_step:          # three launches; whether the step applied is known to the device alone
            self._device_optim_step(grad, grad_scale, ctx=ctx)
        elif self.optimizer == "sgd":   # the momentum buffer lives in exp_avg (exp_avg_sq is unused by this branch)
            _lib.call("mgu_sgd_step", dev, self.flat, grad, self.exp_avg, self.flat.numel(), self.lr, self.momentum, self.wd,
                      self.step_count, grad_scale, ctx=ctx)
        else:
            _lib.call("mgu_adam_step", dev, self.flat, grad, self.exp_avg, self.exp_avg_sq, self.flat.numel(), self.lr, self.betas[0],
                      self.betas[1], self.eps, self.wd, self.step_count, grad_scale, ctx=ctx)
        model.refresh_packed_weights(dev)   # same tensors, new contents: repack in place (no state_dict round trip per step)

    def train_step(self, images: torch.Tensor, masks: torch.Tensor, instances=None) -> torch.Tensor:
        if self._rccl:   # the only data-path collective of the build, issued from inside backward
            loss = self.forward_backward(images, masks, exchange=True, instances=instances)
            self.optimizer_step(1.0)
            return loss
        loss = self.forward_backward(images, masks, instances=instances)
        grad = self.grad
        if self.accumulate > 1:       # every call adds its gradient; the last of each k exchanges the sum and steps
            _lib.call("mgu_grad_accumulate", self.device, self.acc, self.grad, self.acc.numel(), int(self._micro == 0),
                      ctx=self.model._context(self.device))
            self._micro = (self._micro + 1) % self.accumulate
            if self._micro:
                return loss
            grad = self.acc
        scale = allreduce_mean_(grad, self.group) if self.comm is not None else 1.0   # torch.distributed (RCCL / gloo); 1 rank: no-op
        self.optimizer_step(scale / self.accumulate, grad)
        return loss


_CONFIG_OPTIMIZERS = {"adam": "adam", "adamw": "adamw", "sgd": "sgd"}


def trainer_from_config(model: UNet, train_cfg: dict, **overrides) -> "Trainer":
    """Trainer(model, ...) from a training config (configs/training.yaml, as load_config reads it).  The reference's keys:
    optimizer (any letter case, as train_segmentation.py:95-98 lowers it: "Adam", "AdamW", "SGD"), learning_rate, weight_decay,
    sgd_momentum.  Keys of this build, each optional and off when absent: grad_clip_norm (max_grad_norm), ema_decay,
    accumulate_steps (accumulate), skip_nonfinite.  `overrides` are Trainer arguments that win over the config."""
    name = str(train_cfg.get("optimizer", "Adam")).lower()
    if name not in _CONFIG_OPTIMIZERS:
        raise ValueError(f"unsupported optimizer {train_cfg.get('optimizer')!r} in the training config: 'Adam', 'AdamW' or 'SGD'")
    kw = {"optimizer": _CONFIG_OPTIMIZERS[name]}
    for key, arg, conv in (("learning_rate", "lr", float), ("weight_decay", "weight_decay", float), ("sgd_momentum", "momentum", float),
                           ("grad_clip_norm", "max_grad_norm", float), ("ema_decay", "ema_decay", float),
                           ("accumulate_steps", "accumulate", int), ("skip_nonfinite", "skip_nonfinite", bool)):
        if train_cfg.get(key) is not None:
            kw[arg] = conv(train_cfg[key])
    kw.update(overrides)
    return Trainer(model, **kw)


def scheduler_from_config(trainer, train_cfg: dict):
    """The scheduler a training config names under lr_scheduler: "StepLR" (lr_step_size, lr_gamma; train_segmentation.py:105),
    "CosineAnnealingLR" (lr_t_max, default num_epochs; lr_eta_min) or "ReduceLROnPlateau" (lr_factor or lr_gamma, lr_patience);
    None when the key is absent or empty."""
    name = train_cfg.get("lr_scheduler")
    if not name or str(name).lower() == "none":
        return None
    low = str(name).lower()
    if low == "steplr":
        return StepLR(trainer, int(train_cfg.get("lr_step_size", 30)), float(train_cfg.get("lr_gamma", 0.1)))
    if low == "cosineannealinglr":
        t_max = train_cfg.get("lr_t_max", train_cfg.get("num_epochs"))
        if t_max is None:
            raise ValueError("lr_scheduler CosineAnnealingLR needs lr_t_max (or num_epochs) in the training config")
        return CosineAnnealingLR(trainer, int(t_max), float(train_cfg.get("lr_eta_min", 0.0)))
    if low == "reducelronplateau":
        return ReduceLROnPlateau(trainer, factor=float(train_cfg.get("lr_factor", train_cfg.get("lr_gamma", 0.1))),
                                 patience=int(train_cfg.get("lr_patience", 10)))
    raise ValueError(f"unsupported lr_scheduler {name!r} in the training config: 'StepLR', 'CosineAnnealingLR' or 'ReduceLROnPlateau'")


class FlatAdam(_DeviceStep):
    """torch.optim.Adam(params, lr, betas, eps, weight_decay) (the optimizer of both reference loops, train_end_to_end.py:228) for the
    parameters of ANY modules on the HIP path: they are re-homed as views of one flat fp32 buffer, their .grad as views of a flat
    gradient buffer that autograd accumulates into, and step() is one mgu_adam_step launch.  (`Trainer` does the same for the U-Net,
    whose flat order the library fixes; this is the graph branch's half.)"""

    def __init__(self, modules, lr=1e-3, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, exclude=(), decoupled=False, max_grad_norm=0.0,
                 skip_nonfinite=False, ema_decay=0.0, ema_warmup=False):
        """exclude: parameter-name fragments (as in named_parameters()) left out of the flat buffers -- parameters whose .grad stays
        None in the reference loop: torch.optim.Adam skips those entirely (no step count, no weight decay).
        decoupled=True: torch.optim.AdamW.  max_grad_norm, skip_nonfinite, ema_decay, ema_warmup: as Trainer's; with all of them at
        their defaults step() is the one mgu_adam_step launch, otherwise one mgu_optim_step (three launches).  The norm is that of
        THIS optimizer's flat gradient: next to a Trainer (E2ETrainer) each of the two clips its own buffer."""
        self._check_step_options(max_grad_norm, ema_decay)
        seen, params = set(), []
        for m in modules:
            for name, q in m.named_parameters():
                if id(q) not in seen and q.requires_grad and not any(x in name for x in exclude):
                    seen.add(id(q))
                    params.append(q)
        if not params:
            raise RuntimeError("FlatAdam: no parameters to optimize")
        _lib.require_hip(params[0], "FlatAdam")
        self.params, self.device = params, params[0].device
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        n = sum(q.numel() for q in params)
        self.flat = torch.empty(n, device=self.device, dtype=torch.float32)
        self.grad = torch.zeros(n, device=self.device, dtype=torch.float32)
        self.exp_avg = torch.zeros(n, device=self.device, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(n, device=self.device, dtype=torch.float32)
        off = 0
        for q in params:
            k = q.numel()
            self.flat[off:off + k].copy_(q.detach().reshape(-1))
            q.data = self.flat[off:off + k].view_as(q)
            q.grad = self.grad[off:off + k].view_as(q)
            off += k
        self.step_count = 0
        self._init_device_step("adamw" if decoupled else "adam", max_grad_norm, skip_nonfinite, ema_decay, ema_warmup)
        self._alloc_device_step()

    def zero_grad(self) -> None:
        self.grad.zero_()          # the .grad views stay in place (set_to_none would detach them from the flat buffer)

    def step(self, grad_scale: float = 1.0) -> None:
        self.step_count += 1
        if self.device_step:
            self._device_optim_step(self.grad, grad_scale)
        else:
            _lib.call("mgu_adam_step", self.device, self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.flat.numel(), self.lr,
                      self.betas[0], self.betas[1], self.eps, self.wd, self.step_count, grad_scale)
        for q in self.params:      # the kernel wrote the parameters behind torch's back: the packed-weight caches key on _version
            torch.autograd.graph.increment_version(q)


class E2ETrainer:
    """One iteration of scripts/train_end_to_end.py:262-480 on the HIP path, as far as the reference's loss reaches:

        total = L_unet_seg + 0.1 * L_shape (the constant 0, :287) + w_f * L_feature + w_p * L_partition + w_s * L_smooth

    `L_unet_seg` (CrossEntropy of the U-Net logits) is the U-Net's only gradient source -- the script feeds the graph branch torch.randn
    placeholders (:326, :338, :342), not U-Net features -- and goes through `Trainer` (mgu_unet_forward / mgu_cross_entropy /
    mgu_unet_backward).  `L_feature` (FeatureConsistencyLoss on the patch GAT's output, with the batch dimension the script forgets,
    SURVEY appendix A) and `L_partition` (MinCutRefinement) differentiate the patch GAT and the segment predictor through the autograd
    nodes of mgunet.GATNetwork / MinCutRefinement / FeatureConsistencyLoss (mgu_gat_layer_backward, mgu_ncut_backward,
    mgu_feature_consistency_loss_backward).  `L_smooth` is the TV of a constant map (:455) and `L_shape` a constant: their gradient
    is exactly zero and they are not evaluated.
    The whole batch runs as ONE block-diagonal graph (the script loops over the images, :300-437): one patch-GAT launch sequence, one
    segment-predictor sequence and one feature loss for the B images, B normalized-cut nodes (the loss is a per-image quotient, :440).
    Every sub-model of the script's single Adam (:219-229) takes the step: the U-Net in `Trainer`, the patch GAT and the segment
    predictor in `FlatAdam` -- and, when they are handed in, the region GAT, FeatureFusion and DetectionHead too: in the reference
    they hang on the loss through `L_smooth`, whose gradient is zero, so torch gives them zero .grad tensors and Adam still applies
    the L2 term (g = weight_decay * p).
    With more than one rank BOTH flat gradients are averaged over the ranks before the step (the U-Net's by the Trainer's own
    exchange -- torch.distributed or the in-library RCCL buckets -- the graph branch's as one more all-reduce), so every rank holds
    the same parameters after it.  The placeholders are ARGUMENTS here (the script draws them from torch's RNG per image)."""

    def __init__(self, unet_trainer: Trainer, patch_gat: GATNetwork, segment_predictor, mincut, feature_loss, num_segments: int = 2,
                 l_feature_weight: float = 0.1, l_partition_weight: float = 0.5, extra_modules=(),
                 untouched_params=("fc_bbox", "fc_class_scores")):
        """extra_modules: the sub-models the loss does not reach but the script's optimizer holds (region GAT, FeatureFusion,
        DetectionHead, train_end_to_end.py:223-226): stepped with zero gradients, i.e. the weight-decay term alone.
        untouched_params: name fragments of parameters that are NOT on the path to pred_confidence, the one head output the script's
        loss touches (train_end_to_end.py:462) -- DetectionHead.fc_bbox and .fc_class_scores (detection_head.py:57,67): their .grad
        stays None in the reference, so its Adam never steps or decays them, and neither does this one."""
        self.unet = unet_trainer
        self.patch_gat, self.predictor, self.mincut, self.feature_loss = patch_gat, segment_predictor, mincut, feature_loss
        self.K, self.wf, self.wp = num_segments, l_feature_weight, l_partition_weight
        self.extra_modules = [m for m in extra_modules if any(True for _ in m.parameters())]
        self.graph_opt = FlatAdam([patch_gat, segment_predictor, *self.extra_modules], lr=unet_trainer.lr, weight_decay=unet_trainer.wd,
                                  betas=unet_trainer.betas, eps=unet_trainer.eps, exclude=tuple(untouched_params))
        self._batch_graph = None
        self._graphs = {}   # step_images: one PatchGraphConstructor per patch size (its edge lists are cached per shape)

    def _block_diagonal(self, edge_index: torch.Tensor, Np: int, B: int):
        """(edge_index of the B-image batch, graph_ptr): image b's nodes are [b * Np, (b + 1) * Np).  Cached per (edge_index, B)."""
        key = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, Np, B)
        if self._batch_graph is None or self._batch_graph[0] != key:
            off = (torch.arange(B, device=edge_index.device, dtype=edge_index.dtype) * Np).view(B, 1, 1)
            ei = (edge_index.unsqueeze(0) + off).permute(1, 0, 2).reshape(2, -1).contiguous()
            gp = (torch.arange(B + 1, device=edge_index.device, dtype=torch.int64) * Np).to(torch.int32)
            self._batch_graph = (key, ei, gp, edge_index)
        return self._batch_graph[1], self._batch_graph[2]

    @staticmethod
    def exchange_gradients_(unet_grad: torch.Tensor, graph_grad: torch.Tensor, group=None, unet_exchanged: bool = False):
        """Mean all-reduce of both flat gradients over the ranks; returns the factors (1 / world, or 1.0 where nothing is left to
        scale) for the two Adam steps.  `unet_exchanged`: the U-Net gradient already came back averaged (in-library RCCL exchange)."""
        su = 1.0 if unet_exchanged else allreduce_mean_(unet_grad, group)
        sg = allreduce_mean_(graph_grad, group)
        return su, sg

    def step(self, images, masks, patch_features, f_unet_patches, patch_labels, edge_index) -> dict:
        """images (B,3,H,W), masks (B,H,W) int64; per image b (lists of B tensors, or stacked (B, Np, .) tensors): patch_features[b]
        (Np, D_in) -> patch GAT, f_unet_patches[b] (Np, D) and patch_labels[b] (Np,) for L_feature; edge_index: ONE image's patch
        graph (2, E), shared by the batch.  Returns the script's running-loss entries."""
        B = images.shape[0]
        stack = lambda v: v if isinstance(v, torch.Tensor) else torch.stack(list(v), 0)   # noqa: E731
        X, FU, Y = stack(patch_features), stack(f_unet_patches), stack(patch_labels)
        Np = X.shape[1]
        exchange = self.unet._rccl
        loss_seg = self.unet.forward_backward(images, masks, exchange=exchange)
        self.graph_opt.zero_grad()
        ei_all, gp = self._block_diagonal(edge_index, Np, B)
        h = self.patch_gat(X.reshape(B * Np, -1), ei_all, graph_ptr=gp)                               # :332, all images
        lf = self.feature_loss(FU, h.view(B, Np, -1), Y)                                              # :344 (sum over patches, mean over the batch = :440)
        if getattr(self.predictor, "use_gnn", False):
            seg_logits = self.predictor.gnn_predictor(h, ei_all, graph_ptr=gp)                        # :348-351 (:190)
        else:
            seg_logits = self.predictor(h)
        losses, _soft, _hard = self.mincut.forward_batched(h, edge_index, B, self.K, seg_logits.contiguous())
        lp = losses.mean()                                                                            # :441
        (self.wf * lf + self.wp * lp).backward()                                                      # the graph-branch part of :478
        if self.unet.comm is not None:
            su, sg = self.exchange_gradients_(self.unet.grad, self.graph_opt.grad, self.unet.group, unet_exchanged=exchange)
        else:
            su = sg = 1.0
        self.unet.optimizer_step(su)
        self.graph_opt.step(sg)
        total = loss_seg.detach() + self.wf * lf.detach() + self.wp * lp.detach()
        return {"total": total, "l_unet_seg": loss_seg.detach(), "l_shape": torch.zeros((), device=images.device),
                "l_feature": lf.detach(), "l_partition": lp.detach(), "l_smooth": torch.zeros((), device=images.device)}

    def step_images(self, images, masks, images_u8, f_unet_patches, edge_index=None, patch_size: int = 16) -> dict:
        """`step` on inputs derived from the batch itself instead of placeholders: patch_features = patch_node_features(images_u8, p,
        images=images) (scripts/graph_refinement.py:72-113: patch pixel mean x 16 | Sobel mean | equalised-image means, 20 columns),
        patch_labels = patch_labels(masks, p) (the ground-truth form of train_end_to_end.py:340) and, when none is given, edge_index from
        PatchGraphConstructor(p).  images_u8: the batch's (B, H, W, 3) RGB bytes.  f_unet_patches stays an argument: the reference never
        defines it (its width has to equal the patch GAT's output width)."""
        from .patch_inputs import feature_width, patch_labels, patch_node_features
        p = int(patch_size)
        B, _, H, W = images.shape
        want = self.patch_gat.gat_layers[0].heads[0].W.weight.shape[1]
        have = feature_width()
        if want != have:
            raise ValueError(f"the patch GAT takes {want} input features but patch_node_features rows are {have} wide")
        X = patch_node_features(images_u8, p, images=images)
        Y = patch_labels(masks, p, num_classes=self.unet.model.num_classes)
        if edge_index is None:
            edge_index = self._graphs.setdefault(p, PatchGraphConstructor(p)).edge_index(H, W, images.device)
        return self.step(images, masks, X.view(B, -1, have), f_unet_patches, Y, edge_index)
