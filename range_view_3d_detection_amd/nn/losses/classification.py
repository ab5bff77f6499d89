"""Loss configuration objects -- mirror of ``torchbox3d/nn/losses/classification.py:14-119``.

Instantiated from ``conf/model/range_view.yaml:95-99``; on the training path the parameters are
read by ``DetectionHead`` and handed to the fused HIP loss kernel.
"""

from __future__ import annotations

from dataclasses import dataclass

from torch import Tensor

from ..functional import penalty_reduced_focal_loss, sigmoid_focal_loss, varifocal_loss


@dataclass
class VarifocalLoss:
    alpha: float
    gamma: float
    reduction: str

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        return varifocal_loss(input=input, target=target, alpha=self.alpha, gamma=self.gamma, reduction=self.reduction)

    def __call__(self, input: Tensor, target: Tensor) -> Tensor:
        return self.forward(input, target)


@dataclass
class FocalLoss:
    """``torchbox3d/nn/losses/classification.py:57-87``.  The reference's ``forward`` calls ``sigmoid_focal_loss(input, target,
    reduction="none")`` WITHOUT its own ``alpha`` / ``gamma`` (``:83``): the defaults 0.25 and 2 of the published definition apply
    whatever the configuration says.  Reproduced: the fields are kept as configured, ``forward`` and the fused kernel
    (``kernel_alpha`` / ``kernel_gamma``, read by ``DetectionHead``) use 0.25 / 2.0.  The kernel itself takes any ``alpha`` / ``gamma``."""

    alpha: float
    gamma: int
    reduction: str

    kernel_alpha = 0.25
    kernel_gamma = 2.0

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        return sigmoid_focal_loss(input, target, reduction="none")

    def __call__(self, input: Tensor, target: Tensor) -> Tensor:
        return self.forward(input, target)


@dataclass
class PenaltyReducedFocalLoss:
    """``torchbox3d/nn/losses/classification.py:90-119``: the CenterNet-style partner of ``normalize_affinities: true`` (its
    foreground term lives where the soft target is exactly 1)."""

    alpha: float
    gamma: int
    reduction: str

    def forward(self, input: Tensor, target: Tensor) -> Tensor:
        return penalty_reduced_focal_loss(input=input, target=target, alpha=self.alpha, gamma=self.gamma, reduction=self.reduction)

    def __call__(self, input: Tensor, target: Tensor) -> Tensor:
        return self.forward(input, target)
