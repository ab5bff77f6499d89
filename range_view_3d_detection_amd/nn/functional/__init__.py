"""Functional interface -- mirrors ``torchbox3d/nn/functional/__init__.py:8-27``.

On the training path the varifocal term is evaluated INSIDE the fused detection-loss kernel (``csrc/loss.hip``,
``nn/heads/detection_head.py``); this stand-alone ``varifocal_loss`` exists for API parity only and is plain torch ops on
the caller's device (arbitrary shapes) -- it does not call the HIP library and is not on the hot path.
"""

from __future__ import annotations

import torch
from torch import Tensor


def varifocal_loss(input: Tensor, target: Tensor, alpha: float, gamma: float, reduction: str = "none") -> Tensor:
    """``[t>0] t bce + alpha [t==0] sigmoid(x)^gamma bce`` (element-wise, torch ops on the caller's device)."""
    bce = torch.nn.functional.binary_cross_entropy_with_logits(input, target, reduction="none")
    p = input.sigmoid()
    loss = (target > 0.0) * target * bce + alpha * (target == 0) * p.pow(gamma) * bce
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss


def _reduce(loss: Tensor, reduction: str) -> Tensor:
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss


def penalty_reduced_focal_loss(input: Tensor, target: Tensor, alpha: float, gamma: float, reduction: str = "none") -> Tensor:
    """``[t==1] (1-p)^gamma bce + alpha (1-t)^4 p^gamma bce`` (``torchbox3d/nn/functional/__init__.py:30-49``; element-wise, torch ops on
    the caller's device).  The second term runs over every element: at ``t == 1`` it is 0."""
    bce = torch.nn.functional.binary_cross_entropy_with_logits(input, target, reduction="none")
    p = input.sigmoid()
    loss = (target == 1) * (1 - p).pow(gamma) * bce + alpha * (1 - target).pow(4.0) * p.pow(gamma) * bce
    return _reduce(loss, reduction)


def sigmoid_focal_loss(input: Tensor, target: Tensor, alpha: float = 0.25, gamma: float = 2.0, reduction: str = "none") -> Tensor:
    """The published sigmoid focal loss (RetinaNet), soft targets included: ``alpha_t q^gamma bce`` with ``q = p (1-t) + (1-p) t`` and
    ``alpha_t = alpha t + (1-alpha) (1-t)``; ``alpha < 0``: no ``alpha_t`` factor.  Element-wise torch ops on the caller's device."""
    bce = torch.nn.functional.binary_cross_entropy_with_logits(input, target, reduction="none")
    p = input.sigmoid()
    q = p * (1 - target) + (1 - p) * target
    loss = bce * q.pow(gamma)
    if alpha >= 0:
        loss = (alpha * target + (1 - alpha) * (1 - target)) * loss
    return _reduce(loss, reduction)
