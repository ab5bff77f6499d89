"""Training-recipe glue -- mirrors ``torchbox3d/nn/meta/arch.py:48-75`` (``MetaDetector.configure_optimizers``).

The reference builds, through Hydra, ``torch.optim.AdamW(lr=1e-3)`` (``conf/model/range_view.yaml:52-55``) and a
``OneCycleLR`` stepped once per optimisation step (``"interval": "step"``) whose ``max_lr`` is scaled by
``sqrt(num_devices * batch_size)`` when ``use_linear_lr_scaling`` is set (``conf/model/baseline.yaml:25-28``:
``max_lr = 0.00075``, ``batch_size = 4`` per device) and whose ``total_steps`` is the trainer's
``estimated_stepping_batches``.  Lightning calls ``scheduler.step()`` after every ``optimizer.step()``; a plain training
loop (``bench.py``) does the same with the pair returned here.  ``fused=True`` swaps in ``range_view_3d_detection_amd.optim.AdamW``
(same hyper-parameters, state and arithmetic; optional ``max_grad_norm`` = Lightning's ``gradient_clip_val``).

Beyond the shipped recipe: ``weight_decay`` is passed through, ``no_weight_decay_1d`` splits the parameters into the usual two groups
(``ndim >= 2`` with the decay; BatchNorm weights and biases and conv biases, ``ndim <= 1``, with none), and ``params`` may already be a
list of group dicts, taken as torch takes it.  ``OneCycleLR`` gives every group the same scaled ``max_lr``; the fused optimiser steps
all groups in its two launches with one clipping norm.
"""

from __future__ import annotations

import math
from typing import Iterable, List, Tuple

import torch


def one_cycle_max_lr(max_lr: float, num_devices: int, batch_size: int, use_linear_lr_scaling: bool = True) -> float:
    """``max_lr * sqrt(num_devices * batch_size)`` (``arch.py:63-66``); ``batch_size`` is per device."""
    return max_lr * math.sqrt(num_devices * batch_size) if use_linear_lr_scaling else max_lr


def split_no_weight_decay_1d(params: Iterable, weight_decay: float) -> List[dict]:
    """Two parameter groups from an iterable of parameters or of ``named_parameters()`` pairs: ``ndim >= 2`` (conv and linear weights)
    with ``weight_decay``, ``ndim <= 1`` (BatchNorm weights and biases, conv biases) with 0.0; the order within a group is the
    iterable's."""
    decay, no_decay = [], []
    for item in params:
        if isinstance(item, dict):
            raise TypeError("no_weight_decay_1d splits parameters (or named_parameters() pairs); it was given parameter-group dicts")
        p = item[1] if isinstance(item, tuple) else item
        (decay if p.ndim >= 2 else no_decay).append(p)
    return [{"params": decay, "weight_decay": weight_decay}, {"params": no_decay, "weight_decay": 0.0}]


def configure_optimizers(params: Iterable[torch.nn.Parameter], num_devices: int, batch_size: int, total_steps: int,
                         lr: float = 1e-3, max_lr: float = 0.00075, use_linear_lr_scaling: bool = True,
                         debug: bool = False, max_grad_norm: "float | None" = None, fused: bool = False,
                         weight_decay: float = 1e-2, no_weight_decay_1d: bool = False) -> Tuple[torch.optim.Optimizer, "torch.optim.lr_scheduler.LRScheduler | None"]:
    """(AdamW, OneCycleLR stepped per optimisation step) as ``MetaDetector.configure_optimizers`` returns them; in ``debug``
    mode the reference attaches no scheduler (``arch.py:59``).  ``params``: parameters, or group dicts as torch takes them;
    ``no_weight_decay_1d``: parameters or ``named_parameters()`` pairs, split by ``split_no_weight_decay_1d``."""
    params = split_no_weight_decay_1d(params, weight_decay) if no_weight_decay_1d else list(params)
    if fused:  # the same AdamW (and, with max_grad_norm, the recipe's gradient clipping) in two HIP launches: ..optim.AdamW
        from ...optim import AdamW

        optimizer = AdamW(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    else:
        if max_grad_norm is not None:
            raise ValueError("max_grad_norm is folded into the fused optimiser only; call torch.nn.utils.clip_grad_norm_ with torch.optim.AdamW")
        optimizer = torch.optim.AdamW(params, lr=lr, weight_decay=weight_decay)
    if debug:
        return optimizer, None
    scheduler = torch.optim.lr_scheduler.OneCycleLR(optimizer, max_lr=one_cycle_max_lr(max_lr, num_devices, batch_size, use_linear_lr_scaling),
                                                    total_steps=int(total_steps))
    return optimizer, scheduler
