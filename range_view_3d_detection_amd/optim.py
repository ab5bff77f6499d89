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

Weight averaging: ``AveragedModel`` is ``torch.optim.swa_utils.AveragedModel`` (same state-dict keys) whose update is
``rv_average_tensors`` -- one launch -- and, once ``fuse(optimizer, model)`` was called, part of the optimiser's own second launch
(``rv_adamw_step_groups_avg``: the average is formed from the updated parameter while it is in registers).  ``update_bn`` is
``torch.optim.swa_utils.update_bn`` for models that take a batch dict.  DESIGN.md 3.4.
"""

from __future__ import annotations

import itertools
from typing import Any, Dict, Iterable, List, Optional, Tuple

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
        self._averager: Optional["AveragedModel"] = None  # set by AveragedModel.fuse: the step also averages the weights

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

    def _plan(self, ps: List[Tensor], dev, vmax: Optional[List[int]] = None, avg: Optional[List[int]] = None) -> dict:
        """Static part of the device tables for this set of parameters (chunk list, p / m / v / max_exp_avg_sq pointers, the pointers
        of the averaged twins while an ``AveragedModel`` is fused, buffers)."""
        key = tuple((p.data_ptr(), p.numel(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr()) for p in ps)
        if vmax is not None:
            key = (key, tuple(vmax))
        if avg is not None:
            key = (key, "avg", tuple(avg))
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
            if avg is not None:  # so are those of the averaged twins
                plan["avg"] = torch.tensor(avg, dtype=torch.int64).to(dev)
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
        averager = getattr(self, "_averager", None)
        if averager is not None:
            averager._before_fused_step()  # a second fused step without update_parameters() in between: RvError, nothing launched
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
        avg = averager._twin_pointers(ps) if averager is not None else None
        plan = self._plan(ps, dev, vmax, avg)
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
        if len(rows) == 1 and flags[0] == 0 and averager is None:  # the shipped recipe: one group, one step count, nothing special
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
            if averager is not None:  # the same step, and the averaged twin of every stepped parameter from the new value in registers
                L.call("rv_adamw_step_groups_avg", L.ptr(plan["table"]), L.ptr(self._row_column(plan, col, len(rows), dev)),
                       L.ptr(plan.get("vmax")), L.ptr(plan["avg"]), averager._fused_weight(), L.ptr(plan["chunks"]), plan["n_chunks"],
                       L.ptr(plan["partial"]), table, len(rows), max_norm, L.ptr(plan["norm"]), L.stream_ptr())
                averager._after_fused_step(ps)
            else:
                L.call("rv_adamw_step_groups", L.ptr(plan["table"]), L.ptr(self._row_column(plan, col, len(rows), dev)), L.ptr(plan.get("vmax")),
                       L.ptr(plan["chunks"]), plan["n_chunks"], L.ptr(plan["partial"]), table, len(rows), max_norm, L.ptr(plan["norm"]),
                       L.stream_ptr())
        # the kernel wrote the parameters and moments behind torch's back: tell autograd (and everything keyed on
        # Tensor._version, e.g. the packed bf16 weight images of engine.TapLayer) that they changed
        torch.autograd.graph.increment_version(ps)
        self.last_grad_norm = plan["norm"]
        return loss


# ---------------------------------------------------------------------------------------------
# weight averaging (EMA / SWA) and BatchNorm re-estimation: torch.optim.swa_utils on this engine
# ---------------------------------------------------------------------------------------------
def average_weight(n_averaged: int, decay: Optional[float]) -> float:
    """The weight ``w`` of ``averaged = lerp(averaged, current, w)`` for an update that follows ``n_averaged`` earlier ones, as
    ``torch.optim.swa_utils.AveragedModel`` applies it: the first update is a copy (``w = 1``); then ``1 / (n_averaged + 1)`` for the
    equal average (``decay=None``: ``get_swa_multi_avg_fn``) and ``1 - decay`` for the exponential one (``get_ema_multi_avg_fn(decay)``)."""
    if n_averaged < 0:
        raise ValueError(f"n_averaged = {n_averaged}")
    if n_averaged == 0:
        return 1.0
    return 1.0 / (n_averaged + 1) if decay is None else 1.0 - decay


def _reset_count_mirror(module: "AveragedModel", incompatible_keys) -> None:
    module.reset_count_mirror()  # (load_state_dict post hook: n_averaged was just overwritten)


class AveragedModel(torch.optim.swa_utils.AveragedModel):
    """``torch.optim.swa_utils.AveragedModel`` with the update on the device in one launch, or inside the optimiser's step.

    Same constructor, same state-dict keys (``n_averaged``, ``module.*``: checkpoints interchange with torch's class in both directions),
    same arithmetic (``averaged = lerp(averaged, current, w)`` in fp32, ``w`` from ``average_weight``; the first update is a copy).
    ``decay=None`` is torch's default, the equal average (SWA); a float is the exponential average ``get_ema_multi_avg_fn(decay)``.
    The averaged parameters are set ``requires_grad_(False)`` (not part of the state dict): the averaged module is evaluated, never
    trained, and ``engine.prepack_stale()`` -- which re-packs the weight images of every layer that takes gradients at the start of a
    training step -- leaves it alone.

    ``update_parameters(model)`` alone: every fp32 tensor (parameters; BatchNorm's running statistics -- averaged under
    ``use_buffers=True``, copied otherwise) through ``rv_average_tensors``: one launch, two when tensors are averaged AND buffers are
    copied (two weights).  Integer buffers (``num_batches_tracked``) take torch's own expression for them through ``_foreach`` ops.
    ``n_averaged`` is incremented on the device; a host mirror chooses the weight (read from the device once after ``load_state_dict``;
    code that writes ``n_averaged`` by hand calls ``reset_count_mirror()``).  Every tensor a kernel wrote gets its ``_version``
    incremented, which is what keeps the cached weight images and eval folds of the averaged module's layers honest.

    ``fuse(optimizer, model)``: from now on every ``optimizer.step()`` (``optim.AdamW``) is ONE ``rv_adamw_step_groups_avg`` call, which
    also updates the averaged twin of every parameter it steps (8 B per element on top of the step, no separate pass); the following
    ``update_parameters(model)`` completes that update: tensors the step did not cover, buffers, the count, the version bumps.  The
    protocol is strict -- step, update_parameters, step, ... -- and a second fused step before ``update_parameters`` raises ``RvError``
    before anything is launched.  ``update_parameters`` without a pending step is a whole standalone update.  ``unfuse()`` returns the
    optimiser to its own calls (the SWA pattern: start averaging late in the schedule, ``fuse`` then).

    A user-supplied ``avg_fn`` / ``multi_avg_fn``, a ``device`` other than the model's, or a CPU model: torch's own
    ``update_parameters``, unchanged (``decay`` then becomes ``get_ema_multi_avg_fn(decay)``), and ``fuse`` raises ``RvError``.
    Under data parallelism nothing needs a collective: the parameters are identical on all ranks after ``GradSync``, so are the averages."""

    def __init__(self, model: torch.nn.Module, device=None, avg_fn=None, multi_avg_fn=None, use_buffers: bool = False, *,
                 decay: Optional[float] = None) -> None:
        if decay is not None:
            if avg_fn is not None or multi_avg_fn is not None:
                raise ValueError("optim.AveragedModel: decay and avg_fn / multi_avg_fn are exclusive")
            if not 0.0 <= decay <= 1.0:
                raise ValueError(f"Invalid decay value {decay} provided. Please provide a value in [0,1] range.")
        super().__init__(model, device, avg_fn, multi_avg_fn, use_buffers)
        self.decay = None if decay is None else float(decay)
        for p in self.module.parameters():
            p.requires_grad_(False)
        src, own = next(model.parameters(), None), next(self.module.parameters(), None)
        self._native = avg_fn is None and multi_avg_fn is None and src is not None and src.is_cuda and own.device == src.device
        if self._native:
            self.n_averaged = self.n_averaged.to(src.device)  # (torch leaves it on the CPU when `device` is None)
        elif decay is not None:
            self.multi_avg_fn = torch.optim.swa_utils.get_ema_multi_avg_fn(decay)
        self._count: Optional[int] = 0  # host mirror of n_averaged; None: read it from the device at the next use
        # (optimiser, id(parameter) -> averaged twin, the model: in a tuple, so that it is not registered as a submodule; keeps the ids meaningful)
        self._fused: Optional[Tuple[AdamW, Dict[int, Tensor], torch.nn.Module]] = None
        self._pending: Optional[Dict[int, Tensor]] = None  # the twins the last fused step wrote, until update_parameters()
        self._plans: Dict[tuple, dict] = {}
        self.register_load_state_dict_post_hook(_reset_count_mirror)

    # ---- the count ----
    def reset_count_mirror(self) -> None:
        self._count = None

    def _n(self) -> int:
        if self._count is None:
            self._count = int(self.n_averaged)
        return self._count

    # ---- the optimiser's side of the fuse protocol (optim.AdamW.step) ----
    def fuse(self, optimizer: AdamW, model: torch.nn.Module) -> None:
        if not self._native:
            raise L.RvError("optim.AveragedModel.fuse: this averaged model takes torch's update_parameters path (a custom avg_fn / "
                            "multi_avg_fn, another device, or a CPU model): there is nothing to fuse")
        if not isinstance(optimizer, AdamW):
            raise L.RvError("optim.AveragedModel.fuse: the optimiser must be range_view_3d_detection_amd.optim.AdamW")
        if getattr(optimizer, "_averager", None) not in (None, self) or (self._fused is not None and self._fused[0] is not optimizer):
            raise L.RvError("optim.AveragedModel.fuse: one optimiser and one averaged model at a time (unfuse() first)")
        if self._pending is not None:
            raise L.RvError("optim.AveragedModel.fuse: a fused step is waiting for update_parameters()")
        twins: Dict[int, Tensor] = {}
        for a, p in zip(self.module.parameters(), model.parameters()):  # by the order of parameters(), as torch zips them
            if a.shape != p.shape or a.dtype != torch.float32 or p.dtype != torch.float32 or a.device != p.device or not a.is_contiguous():
                raise L.RvError("optim.AveragedModel.fuse: the averaged twin of a parameter must be a contiguous fp32 tensor of its shape on its device")
            twins[id(p)] = a.detach()
        self._fused = (optimizer, twins, model)
        optimizer._averager = self

    def unfuse(self) -> None:
        if self._pending is not None:
            raise L.RvError("optim.AveragedModel.unfuse: a fused step is waiting for update_parameters()")
        if self._fused is not None:
            self._fused[0]._averager = None
        self._fused = None

    def _before_fused_step(self) -> None:
        if self._pending is not None:
            raise L.RvError("optim.AdamW.step: the previous fused step already averaged the weights; call update_parameters(model) of the "
                            "fused AveragedModel between two steps")

    def _twin_pointers(self, ps: List[Tensor]) -> List[int]:
        twins = self._fused[1]
        return [twins[id(p)].data_ptr() if id(p) in twins else 0 for p in ps]

    def _fused_weight(self) -> float:
        return average_weight(self._n(), self.decay)

    def _after_fused_step(self, ps: List[Tensor]) -> None:
        twins = self._fused[1]
        self._pending = {id(p): twins[id(p)] for p in ps if id(p) in twins}

    # ---- the update ----
    def _plan(self, pairs: List[Tuple[Tensor, Tensor]], dev) -> dict:
        """Device table (avg, src, n) and chunk list of ``rv_average_tensors`` for these (averaged, current) pairs; uploaded once."""
        key = tuple((a.data_ptr(), p.data_ptr(), a.numel()) for a, p in pairs)
        plan = self._plans.get(key)
        if plan is None:
            ce = int(L.load().rv_optim_chunk_elems())
            chunks = [(i, c) for i, (a, _) in enumerate(pairs) for c in range((a.numel() + ce - 1) // ce)]
            if len(self._plans) >= 4:  # (parameters + buffers, buffers alone, parameters alone: a training loop alternates between few)
                self._plans.clear()
            plan = {"table": torch.tensor(key, dtype=torch.int64).reshape(-1, 3).to(dev), "chunks": torch.tensor(chunks, dtype=torch.int32).to(dev),
                    "n_chunks": len(chunks)}
            self._plans[key] = plan
        return plan

    def _launch(self, pairs: List[Tuple[Tensor, Tensor]], w: float, dev) -> None:
        pairs = [(a, p) for a, p in pairs if a.numel() > 0]
        if not pairs:
            return
        plan = self._plan(pairs, dev)
        L.call("rv_average_tensors", L.ptr(plan["table"]), L.ptr(plan["chunks"]), plan["n_chunks"], w, L.stream_ptr())

    @torch.no_grad()
    def update_parameters(self, model: torch.nn.Module) -> None:
        if not self._native:
            return super().update_parameters(model)
        n = self._n()
        w = average_weight(n, self.decay)
        done, self._pending = self._pending or {}, None
        dev = self.n_averaged.device
        averaged: List[Tuple[Tensor, Tensor]] = []  # fp32 (averaged, current) pairs that take the weight w
        copied: List[Tuple[Tensor, Tensor]] = []  # fp32 buffers kept in step with the model (use_buffers=False): w = 1
        ints: List[Tuple[Tensor, Tensor]] = []  # non-floating buffers
        if not done or len(done) < len(self._fused[1]):  # (a fused step that covered every parameter of the map: nothing left to find)
            for a, p in zip(self.module.parameters(), model.parameters()):
                if id(p) not in done:
                    averaged.append((a.detach(), p.detach()))
        for a, b in zip(self.module.buffers(), model.buffers()):
            (ints if not (a.is_floating_point() or a.is_complex()) else averaged if self.use_buffers else copied).append((a, b.detach()))
        for a, p in averaged + copied:
            if not (a.dtype == torch.float32 and p.dtype == torch.float32 and a.is_cuda and a.device == p.device and a.shape == p.shape
                    and a.is_contiguous() and p.is_contiguous()):
                raise L.RvError("optim.AveragedModel: floating-point tensors must be contiguous fp32 CUDA tensors on one device, of equal "
                                "shape on both sides (no CPU fallback)")
        if w == 1.0:  # the first update, a copy of everything: one launch
            self._launch(averaged + copied, 1.0, dev)
        else:
            self._launch(averaged, w, dev)
            self._launch(copied, 1.0, dev)
        if ints:
            ia, ib = [a for a, _ in ints], [b.to(a.device) for a, b in ints]
            if n == 0 or not self.use_buffers:
                torch._foreach_copy_(ia, ib)
            else:
                # torch's expression for a non-floating tensor, element-wise and therefore on ONE flat tensor per side when the dtypes
                # agree (num_batches_tracked of every BatchNorm: the foreach ops take integer tensors one by one): a few launches
                flat = len({a.dtype for a in ia} | {b.dtype for b in ib}) == 1
                xa, xb = ([torch.cat([a.reshape(-1) for a in ia])], [torch.cat([b.reshape(-1) for b in ib])]) if flat else (ia, ib)
                if self.decay is not None:  # get_ema_multi_avg_fn: copy_(p_ema * decay + p_model * (1 - decay)), formed in fp32
                    out = torch._foreach_add(torch._foreach_mul(xa, self.decay), torch._foreach_mul(xb, 1 - self.decay))
                else:  # get_swa_avg_fn: copy_(averaged + (current - averaged) / (n + 1)), the quotient and the sum in fp32
                    out = torch._foreach_add(xa, torch._foreach_div(torch._foreach_sub(xb, xa), float(n + 1)))
                if flat:
                    out = [o.view(a.shape) for o, a in zip(out[0].split([a.numel() for a in ia]), ia)]
                torch._foreach_copy_(ia, out)  # (the copy truncates, as copy_ into the integer buffer does)
        self.n_averaged += 1
        self._count = n + 1
        # the kernels wrote these behind torch's back (the fused step's twins among them): tell everything keyed on Tensor._version
        written = [a for a, _ in averaged + copied] + list(done.values())
        if written:
            torch.autograd.graph.increment_version(written)


def _to_device(x: Any, device) -> Any:
    if isinstance(x, Tensor):
        return x.to(device)
    if isinstance(x, dict):
        return {k: _to_device(v, device) for k, v in x.items()}
    return x


@torch.no_grad()
def update_bn(loader: Iterable[Any], model: torch.nn.Module, device=None) -> None:
    """``torch.optim.swa_utils.update_bn``: reset the running statistics of every BatchNorm of ``model``, re-estimate them as the
    cumulative average over one pass of ``loader`` (train-mode forwards under ``no_grad``), restore the momenta and the mode.

    A batch is what the model takes -- the detector's batch dict, or a tensor --, or a list / tuple whose first element is that (torch's
    rule); ``device``: tensors (also those in a dict) are moved there first.  The cumulative average needs no device read here: before the
    k-th batch every BatchNorm's ``momentum`` is the host float ``1 / k``, which equals ``1 / (num_batches_tracked + 1)`` after the reset.
    (torch's own ``update_bn`` sets ``momentum = None`` instead, which the engine honours with one read of the counters per program.)"""
    momenta = {}
    for module in model.modules():
        if isinstance(module, torch.nn.modules.batchnorm._BatchNorm):
            module.reset_running_stats()
            momenta[module] = module.momentum
    if not momenta:
        return
    was_training = model.training
    model.train()
    try:
        for k, batch in enumerate(loader, 1):
            if isinstance(batch, (list, tuple)):
                batch = batch[0]
            if device is not None:
                batch = _to_device(batch, device)
            for module in momenta:
                module.momentum = 1.0 / k
            model(batch)
    finally:
        for module, momentum in momenta.items():
            module.momentum = momentum
        model.train(was_training)
