"""Launchers of csrc/bw2.hip: the eval-mode passes between badwinner2's
convolutions (acfe_mag_rownorm, acfe_leaky_bn) and acfe_softmax.  Inference
only: none of them is an autograd node.  acfe.ops re-exports them."""
from __future__ import annotations

import torch

from ._lib import call
from ._torch import dtype_code, ptr, stream

F32 = torch.float32


def softmax(z: torch.Tensor) -> torch.Tensor:
    """Row softmax of fp32 logits [B, L] (acfe_softmax; badwinner2.py:321)."""
    B, L = z.shape
    z = z.contiguous()
    p = torch.empty_like(z)
    call("acfe_softmax", ptr(z), B, L, ptr(p), stream())
    return p


def mag_rownorm(mel: torch.Tensor, a: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, out_dtype, eps=1e-3):
    """MagTransform + the eval-mode BatchNormalization over the mel axis
    (badwinner2.py:230-233) of the fp32 mel power [B, M, T] -> [B, M, T] in
    out_dtype (acfe_mag_rownorm).  Inference only: no autograd node."""
    if mel.dtype != F32 or mel.dim() != 3:
        raise TypeError("mag_rownorm takes the fp32 mel [B, M, T]")
    B, M, T = mel.shape
    if a.numel() != 1 or mean.shape != (M,) or var.shape != (M,):
        raise ValueError(f"mag_rownorm: a [1], mean / var [{M}] expected")
    mel = mel.contiguous()
    y = torch.empty((B, M, T), dtype=out_dtype, device=mel.device)
    call("acfe_mag_rownorm", ptr(mel), B, M, T, ptr(a), ptr(mean), ptr(var), float(eps), ptr(y),
         dtype_code(out_dtype), stream())
    return y


def leaky_bn(x: torch.Tensor, alpha: float, scale: torch.Tensor | None = None, shift: torch.Tensor | None = None,
             out: torch.Tensor | None = None):
    """scale[c] * LeakyReLU(alpha)(x) + shift[c] over NHWC x (acfe_leaky_bn): the
    eval-mode LeakyReLU -> BatchNormalization pairs of badwinner2.py:236-297;
    without scale / shift the bare LeakyReLU of :307.  out: the result's
    tensor, x itself for in place.  Inference only: no autograd node."""
    C = x.shape[-1]
    if not x.is_contiguous():
        raise ValueError("leaky_bn takes a contiguous NHWC tensor")
    if (scale is None) != (shift is None):
        raise ValueError("leaky_bn: scale and shift go together")
    if scale is not None and not (scale.dtype == shift.dtype == F32 and scale.shape == shift.shape == (C,)):
        raise ValueError(f"leaky_bn: fp32 scale / shift [{C}] expected")
    y = torch.empty_like(x) if out is None else out
    if y.shape != x.shape or y.dtype != x.dtype or not y.is_contiguous():
        raise ValueError("leaky_bn: out must match x")
    call("acfe_leaky_bn", ptr(x), x.numel() // C, C, float(alpha), ptr(scale), ptr(shift), ptr(y),
         dtype_code(x.dtype), stream())
    return y
