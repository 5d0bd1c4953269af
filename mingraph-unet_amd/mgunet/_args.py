"""The checks and views of tensor arguments that more than one module needs, each written once: the NHWC storage behind an NCHW
view, an integer map as a batch, an evaluator's device, and the preamble every evaluator's update() runs on its batch.  Pure
Python / torch: importable, and testable, without a HIP device."""
from __future__ import annotations

import torch

from . import _lib


def nhwc_storage(x: torch.Tensor) -> torch.Tensor:
    """The contiguous (B, H, W, C) tensor behind the (B, C, H, W) view x: x's own storage (same data_ptr(), no kernel) when it is
    stored NHWC, as every UNet.forward output is; otherwise one copy."""
    return x.permute(0, 2, 3, 1).contiguous()   # .contiguous() returns its argument when there is nothing to do


def batched_map(x: torch.Tensor, what: str) -> torch.Tensor:
    """The integer (H, W) or (B, H, W) map x as (B, H, W): an (H, W) map is a batch of one."""
    if x.is_floating_point() or x.dtype == torch.bool or x.dim() not in (2, 3):
        raise TypeError(f"{what} must be an integer (H, W) or (B, H, W) tensor")
    return x.reshape((1,) + tuple(x.shape)) if x.dim() == 2 else x


def resolve_device(device, who: str) -> torch.device:
    """torch.device(device), which must be a HIP device; one without an index is the current device."""
    device = torch.device(device)
    _lib.require_hip(device, who)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def check_masks(masks: torch.Tensor, B: int, H: int, W: int) -> None:
    """Raise unless masks is (B, H, W), the batch and image size of the logits it belongs to."""
    if tuple(masks.shape) != (B, H, W):
        raise ValueError(f"masks shape {tuple(masks.shape)} does not match logits {(B, H, W)}")


def logits_and_masks(logits_nchw: torch.Tensor, masks: torch.Tensor, device: torch.device, num_classes: int):
    """(NHWC logits, int64 masks on the device, B, H, W, C) of an evaluator's update(logits, masks), checked: float32 (B, C, H, W)
    logits on `device` with C == num_classes, masks of shape (B, H, W)."""
    if not logits_nchw.is_cuda or logits_nchw.device != device:
        raise RuntimeError(f"logits must live on {device}")
    if logits_nchw.dtype != torch.float32 or logits_nchw.dim() != 4:
        raise TypeError("expected (B, C, H, W) float32 logits")
    B, C, H, W = logits_nchw.shape
    if C != num_classes:
        raise ValueError(f"logits have {C} classes, the evaluator {num_classes}")
    check_masks(masks, B, H, W)
    return nhwc_storage(logits_nchw), masks.to(device, torch.int64).contiguous(), B, H, W, C
