"""Launcher of acfe_loss_weighted (csrc/loss_weighted.hip): the Keras loss with
fit(class_weight=...) and label_smoothing (reference audiomodel.py:523-562,
:1206-1223).  acfe.ops.loss_and_grad comes here when either option is set; with
both at their defaults it stays on acfe_loss."""
from __future__ import annotations

import torch

from ._lib import call
from ._torch import ptr, stream

F32 = torch.float32


def check_class_weights(class_weights, L, device):
    """A 1-D float32 tensor of length L on `device` (its values, finite and
    >= 0, are the caller's to check on the host before the upload)."""
    if not isinstance(class_weights, torch.Tensor) or class_weights.dtype != F32:
        raise TypeError("class_weights must be a float32 tensor")
    if class_weights.dim() != 1 or class_weights.shape[0] != L:
        raise ValueError(f"class_weights must have shape ({L},), got {tuple(class_weights.shape)}")
    if class_weights.device != device:
        raise ValueError(f"class_weights are on {class_weights.device}, the logits on {device}")
    return class_weights.contiguous()


def weighted_loss_and_grad(logits, target, mode_code, grad_scale, class_weights, label_smoothing):
    """(loss[1], dL/dlogits) of acfe_loss_weighted: two launches, no host
    synchronisation.  mode_code: 0 BCE, 1 CCE."""
    B, L = logits.shape
    if class_weights is not None:
        class_weights = check_class_weights(class_weights, L, logits.device)
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
    loss = torch.empty((1,), dtype=F32, device=logits.device)
    dz = torch.empty_like(logits)
    row_loss = torch.empty((B,), dtype=F32, device=logits.device)
    call("acfe_loss_weighted", ptr(logits.contiguous()), ptr(target.contiguous().to(F32)), B, L, mode_code, grad_scale,
         ptr(class_weights), label_smoothing, ptr(loss), ptr(dz), ptr(row_loss), None, stream())
    return loss, dz
