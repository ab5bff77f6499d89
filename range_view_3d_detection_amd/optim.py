"""``AdamW`` with the step of ALL parameters of ALL parameter groups in two HIP launches (``rv_adamw_step`` / ``rv_adamw_step_groups``).

Drop-in for ``torch.optim.AdamW`` where the reference instantiates its optimiser (``conf/model/range_view.yaml:52-55`` ->
``nn/meta/arch.py:57``, ``_target_: torch.optim.AdamW``): same constructor keywords, same ``param_groups`` (so ``OneCycleLR``
drives ``lr`` and -- ``cycle_momentum`` -- ``betas`` of every group exactly as it does torch's), same ``state`` keys (``step``,
``exp_avg``, ``exp_avg_sq``, and ``max_exp_avg_sq`` under ``amsgrad``), same arithmetic operation by operation in fp32
(torch/optim/adam.py, foreach path), so ``state_dict()`` / ``load_state_dict()`` interchange with torch's in both directions.

Covered, as torch does it: several parameter groups with their own ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` / ``amsgrad`` /
``maximize`` (the "no weight decay on BatchNorm and biases" split, a lower rate for a pretrained backbone); parameters without a
gradient are skipped and their ``state["step"]`` does not advance, and every parameter is bias-corrected with ITS OWN step count
(a frozen-then-unfrozen backbone, an unused tower).  ``foreach`` and ``fused`` are accepted and ignored (this optimiser is its own
fused form).  Still refused: ``capturable=True`` and ``differentiable=True`` (``NotImplementedError``: the step count is a host
scalar and the update is not recorded by autograd), and more distinct (group, step count) pairs in one step than
``rv_adam_max_rows()`` (``RvError``).

One extra keyword: ``max_grad_norm`` folds ``torch.nn.utils.clip_grad_norm_(all parameters, max_grad_norm)`` (Lightning's
``gradient_clip_val: 35.0``, ``conf/trainer/train.yaml``) into the same two launches: ONE norm over the gradients of all groups, the
gradients scaled on the fly, ``p.grad`` left as the backward pass wrote it; the total norm of the last step is
``optimizer.last_grad_norm`` (a device scalar, no host sync).

A step with one group, one step count, no amsgrad and no maximize -- the shipped recipe -- is the ``rv_adamw_step`` call it always was;
anything else is ONE ``rv_adamw_step_groups`` call: the hyper-parameters of every (group, step count) present travel as rows in the
kernel's arguments, and a device column names the row of each tensor (re-uploaded only when it changes).

No CPU fallback: parameters must be fp32 CUDA tensors on one device (``RvError`` otherwise).
"""

from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L


def _validate(lr, betas, eps, weight_decay) -> None:
    if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not 0.0 <= weight_decay:
        raise ValueError("invalid AdamW hyper-parameter")


class AdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, amsgrad: bool = False, max_grad_norm: Optional[float] = None, *, maximize: bool = False,
                 foreach: Optional[bool] = None, capturable: bool = False, differentiable: bool = False, fused: Optional[bool] = None) -> None:
        if capturable:
            raise NotImplementedError("capturable=True: the step count of optim.AdamW is a host scalar (the bias corrections are formed on the host)")
        if differentiable:
            raise NotImplementedError("differentiable=True: the fused update writes the parameters in place and is not recorded by autograd")
        _validate(lr, betas, eps, weight_decay)
        # the keys torch.optim.AdamW's groups carry, so that a state_dict of either loads into the other (`foreach` / `fused`
        # are accepted and not kept: this optimiser is its own fused form, and a torch optimiser that loads the groups keeps its default)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad), maximize=bool(maximize),
                                      foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True))
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm: Optional[Tensor] = None
        self._plans: Dict[tuple, dict] = {}

    def __setstate__(self, state) -> None:
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)
            group.setdefault("maximize", False)

    def _init_state(self, p: Tensor, amsgrad: bool = False) -> dict:
        st = self.state[p]
        if not st:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise L.RvError("range_view_3d_detection_amd.optim.AdamW: parameters must be contiguous fp32 CUDA tensors (no CPU fallback)")
            st["step"] = torch.tensor(0.0, dtype=torch.float32)  # host scalar, as torch keeps it on the non-capturable path
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if amsgrad and "max_exp_avg_sq" not in st:
            st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _plan(self, ps: List[Tensor], dev, vmax: Optional[List[int]] = None) -> dict:
        """Static part of the device tables for this set of parameters (chunk list, p / m / v / max_exp_avg_sq pointers, buffers)."""
        key = tuple((p.data_ptr(), p.numel(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr()) for p in ps)
        if vmax is not None:
            key = (key, tuple(vmax))
        plan = self._plans.get(key)
        if plan is None:
            ce = int(L.load().rv_optim_chunk_elems())
            tens = np.zeros((len(ps), 5), dtype=np.int64)  # (p, g, m, v, n) per tensor = struct OptTensor
            chunks = []
            for i, p in enumerate(ps):
                st = self.state[p]
                tens[i] = (p.data_ptr(), 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
                chunks += [(i, c) for c in range((p.numel() + ce - 1) // ce)]
            ch = torch.tensor(chunks, dtype=torch.int32).to(dev)
            self._plans.clear()
            plan = {"tens": tens, "host": torch.empty((len(ps), 5), dtype=torch.int64).pin_memory(), "chunks": ch, "n_chunks": len(chunks),
                    "partial": torch.empty(len(chunks), dtype=torch.float32, device=dev),
                    "table": torch.empty((len(ps), 5), dtype=torch.int64, device=dev),
                    "norm": torch.zeros(1, dtype=torch.float32, device=dev)}
            if vmax is not None:  # the max_exp_avg_sq pointers are part of the key: uploaded once
                plan["vmax"] = torch.tensor(vmax, dtype=torch.int64).to(dev)
            self._plans[key] = plan
        return plan

    def _row_column(self, plan: dict, col: np.ndarray, n_rows: int, dev) -> Tensor:
        """The device column ``tensor_row`` of the plan holding ``col``; uploaded (pinned staging, an event) only when it changed."""
        if col.min() < 0 or col.max() >= n_rows:  # the kernel indexes an array in its own arguments with these
            raise L.RvError(f"optim.AdamW: a row index outside 0 .. {n_rows - 1}")
        if plan.get("row_col") is None or not np.array_equal(plan["row_col"], col):
            if plan.get("row_dev") is None:
                plan["row_host"] = torch.empty(len(col), dtype=torch.int32).pin_memory()
                plan["row_dev"] = torch.empty(len(col), dtype=torch.int32, device=dev)
            else:
                plan["row_copied"].synchronize()  # (the earlier upload has long finished; this makes the reuse of the pinned buffer exact)
            plan["row_host"].copy_(torch.from_numpy(col))
            plan["row_dev"].copy_(plan["row_host"], non_blocking=True)
            plan["row_copied"] = torch.cuda.Event()
            plan["row_copied"].record()
            plan["row_col"] = col
        return plan["row_dev"]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ps: List[Tensor] = []
        owner: List[int] = []  # the group of each parameter of `ps`
        for gi, group in enumerate(self.param_groups):
            _validate(group["lr"], group["betas"], group["eps"], group["weight_decay"])
            if group.get("capturable") or group.get("differentiable"):
                raise NotImplementedError("optim.AdamW: capturable / differentiable parameter groups are not supported")
            for p in group["params"]:
                if p.grad is None:
                    continue
                self._init_state(p, bool(group["amsgrad"]))
                g = p.grad
                if g.is_sparse or g.dtype != torch.float32 or not g.is_cuda:
                    raise L.RvError("range_view_3d_detection_amd.optim.AdamW: gradients must be dense fp32 CUDA tensors")
                if not g.is_contiguous():
                    p.grad = g.contiguous()
                ps.append(p)
                owner.append(gi)
        if not ps:
            return loss
        dev = ps[0].device
        if any(p.device != dev for p in ps):
            raise L.RvError("range_view_3d_detection_amd.optim.AdamW: one launch covers all parameters, so they must be on one device")
        # torch.optim.AdamW bias-corrects every parameter with ITS OWN step count, and every group has its own hyper-parameters:
        # one row per distinct (group, step count) present in this step, in order of first appearance (host scalars: no device sync)
        rows: Dict[Tuple[int, int], int] = {}
        col = np.empty(len(ps), dtype=np.int32)
        for i, (p, gi) in enumerate(zip(ps, owner)):
            col[i] = rows.setdefault((gi, int(self.state[p]["step"]) + 1), len(rows))
        flags = [(L.ADAM_AMSGRAD if self.param_groups[gi]["amsgrad"] else 0) | (L.ADAM_MAXIMIZE if self.param_groups[gi]["maximize"] else 0)
                 for gi, _ in rows]
        max_rows = int(L.load().rv_adam_max_rows())
        if len(rows) > max_rows:
            raise L.RvError(f"optim.AdamW: {len(rows)} distinct (parameter group, step count) pairs in one step, more than "
                            f"rv_adam_max_rows() = {max_rows}")
        any_amsgrad = any(f & L.ADAM_AMSGRAD for f in flags)
        vmax = [self.state[p]["max_exp_avg_sq"].data_ptr() if self.param_groups[gi]["amsgrad"] else 0 for p, gi in zip(ps, owner)] if any_amsgrad else None
        plan = self._plan(ps, dev, vmax)
        tens = plan["tens"]
        tens[:, 1] = [p.grad.data_ptr() for p in ps]  # the only per-step part of the table
        if plan.get("copied") is not None:
            plan["copied"].synchronize()  # (the previous step's upload has long finished; this makes the reuse of the pinned buffer exact)
        plan["host"].copy_(torch.from_numpy(tens))
        plan["table"].copy_(plan["host"], non_blocking=True)
        plan["copied"] = torch.cuda.Event()
        plan["copied"].record()
        for p in ps:
            self.state[p]["step"] += 1
        max_norm = float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0
        if len(rows) == 1 and flags[0] == 0:  # the shipped recipe: one group, one step count, nothing special
            (gi, step), = rows
            group = self.param_groups[gi]
            beta1, beta2 = group["betas"]
            L.call("rv_adamw_step", L.ptr(plan["table"]), L.ptr(plan["chunks"]), plan["n_chunks"], L.ptr(plan["partial"]),
                   float(group["lr"]), float(beta1), float(beta2), float(group["eps"]),
                   float(group["weight_decay"]), step, max_norm,
                   L.ptr(plan["norm"]), L.stream_ptr())
        else:
            table = (L.AdamRow * len(rows))()
            for r, ((gi, step), f) in enumerate(zip(rows, flags)):
                group = self.param_groups[gi]
                table[r] = L.AdamRow(float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                                     float(group["weight_decay"]), step, f)
            L.call("rv_adamw_step_groups", L.ptr(plan["table"]), L.ptr(self._row_column(plan, col, len(rows), dev)), L.ptr(plan.get("vmax")),
                   L.ptr(plan["chunks"]), plan["n_chunks"], L.ptr(plan["partial"]), table, len(rows), max_norm, L.ptr(plan["norm"]),
                   L.stream_ptr())
        # the kernel wrote the parameters and moments behind torch's back: tell autograd (and everything keyed on
        # Tensor._version, e.g. the packed bf16 weight images of engine.TapLayer) that they changed
        torch.autograd.graph.increment_version(ps)
        self.last_grad_norm = plan["norm"]
        return loss
