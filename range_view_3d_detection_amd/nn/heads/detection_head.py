"""``DetectionHead`` -- mirrors ``torchbox3d/nn/heads/detection_head.py:42-449``.

Same constructor keywords (``conf/model/range_view.yaml:88-126``), same sub-module names
(``classification_head.{stride}.{task}`` / ``regression_head...`` => same state-dict keys) and the
same ``forward(input, data, return_loss) -> (multiscale_outputs, losses)`` contract, including
the side effect of writing the per-stride target dicts into ``data`` (``:197-198``).

What runs where: the towers are fused HIP tap-conv programs; target assignment
(``compute_targets`` :496-665) and the soft-target / varifocal / L1 loss (:202-449,
``math/ops/assignment.py:76-161``) are device kernels without host synchronisation (the
reference loops over sweeps, tasks and instances in Python with ``.unique()/.tolist()``).

Any list of FPN strides and any number of tasks: one level of stride 1 with one task (the shipped rv-* / base-* recipes) runs the
one-level entry points (``rv_assign_targets``, ``rv_detection_loss_*``); every other layout, and ``fpn_assignment_method: RANGE``,
runs the multi-level ones (``rv_assign_targets_multilevel``, ``rv_detection_loss_multilevel_*``), which assign all levels and tasks
in one sequence of launches and normalise every level by the foreground / object counts summed over all of them.
``fpn_assignment_method: POINTS`` raises: the reference overwrites its configured intervals with constants (``:583``).

Soft target assignment takes every option of ``targets_config`` (``math/ops/assignment.py:76-147``): ``affinity_fn`` GAUSSIAN | BEV,
``normalize_affinities`` and ``k`` (``.inf`` or an integer).  GAUSSIAN without normalisation and ``k = inf`` (every shipped recipe) is a
per-pixel map inside the loss kernels, as before; any other combination runs ``rv_soft_assign`` (per-instance minimum / top-k threshold
on the device, no host synchronisation) inside the loss node and the ``rv_detection_loss_multilevel_*_aff`` pair, see ``soft_options``.

Both loss slots follow the configuration: ``_cls_loss`` VarifocalLoss | FocalLoss | PenaltyReducedFocalLoss, ``_regression_loss``
``torch.nn.L1Loss`` | ``SmoothL1Loss`` | ``HuberLoss`` | ``MSELoss`` (``reduction: none``).  Varifocal + L1 (every shipped recipe) takes the
routes above unchanged; any other pair runs the same table node on ``rv_detection_loss_table_*`` (``rvLossKinds``, include/rv3d.h).
"""

from __future__ import annotations

import ctypes
import importlib
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor, nn

from ... import _lib as L
from ...engine import _require_cuda
from .dense_head import DenseHead, forward_pair

COLS = ("tx_m", "ty_m", "tz_m", "length_m", "width_m", "height_m", "qw", "qx", "qy", "qz", "task_id", "offset", "batch_index")
FOCAL_PRIOR_PROB = 0.01


def _cfg_get(cfg: Any, key: str, default: Any = None) -> Any:
    if isinstance(cfg, Mapping):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def annotations_to_cuboids(annotations: Any) -> np.ndarray:
    """Annotation table -> (M,10) fp64 [x,y,z,l,w,h,yaw,task,offset,batch] (``utils/polars.py:9-22``).

    Accepts a polars frame (``select(COLS).to_numpy()``), a numpy array or a tensor of shape (M,13).
    """
    if isinstance(annotations, Tensor):
        arr = annotations.detach().cpu().numpy()
    elif hasattr(annotations, "select"):
        arr = annotations.select(list(COLS)).to_numpy()
    else:
        arr = np.asarray(annotations)
    arr = np.asarray(arr, dtype=np.float64).reshape(-1, 13)
    if arr.shape[0] == 0:
        return np.zeros((0, 10), dtype=np.float64)
    w, x, y, z = arr[:, 6], arr[:, 7], arr[:, 8], arr[:, 9]
    yaw = np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
    return np.concatenate([arr[:, :6], yaw[:, None], arr[:, 10:]], axis=1)


def _partition(targets_config: Any, stride: Any) -> Tuple[float, float]:
    parts = _cfg_get(targets_config, "range_partitions")
    for key in (stride, int(stride), str(stride)):
        try:
            lower, upper = parts[key]
            return float(lower), float(upper)
        except (KeyError, TypeError, IndexError):
            continue
    raise KeyError(f"targets_config.range_partitions has no entry for stride {stride}")


def _assignment_method(targets_config: Any) -> Optional[str]:
    method = _cfg_get(targets_config, "fpn_assignment_method")
    if method is None or method == "RANGE":
        return method
    if method == "POINTS":
        raise NotImplementedError("fpn_assignment_method POINTS: the reference overwrites the configured point_intervals with "
                                  "constants (detection_head.py:583), so the configuration does not say what it computes")
    raise ValueError(f"unknown fpn_assignment_method {method!r}")


def soft_options(targets_config: Any) -> Tuple[int, bool, int]:
    """``(affinity_fn, normalize_affinities, k)`` of ``targets_config`` as ``rv_soft_assign`` takes them (``L.AFFINITY_*``, bool, 0 = inf).

    ``affinity_fn`` is case-insensitive; an unknown name raises as the reference does (``assignment.py:96-102``).  ``k`` is ``inf`` or an
    integer-valued number >= 1.  ``BEV`` with ``normalize_affinities`` is a ``ValueError``: the reference's ``iou_2d_axis_aligned`` divides
    a name that does not exist there (``assignment.py:71-72``, an ``UnboundLocalError``).

    Ties at the k-th value, which ``torch.topk`` leaves open: a pixel stays iff its affinity is >= the instance's ``min(k, |set|)``-th
    largest affinity (and != 0) -- a per-instance threshold, independent of pixel order; equal to the reference whenever the k-th and
    (k+1)-th values differ.  The instance's set is ``panoptics == p``, whatever ``mask`` says there."""
    name = str(_cfg_get(targets_config, "affinity_fn", "GAUSSIAN")).upper()
    if name not in ("GAUSSIAN", "BEV"):
        raise NotImplementedError("This affinity function is not implemented.")
    normalize = bool(_cfg_get(targets_config, "normalize_affinities", False))
    if name == "BEV" and normalize:
        raise ValueError("affinity_fn BEV with normalize_affinities: the reference fails there with an UnboundLocalError "
                         "(math/ops/assignment.py:71-72 divides `object_ious`, which iou_2d_axis_aligned never binds)")
    k = _cfg_get(targets_config, "k", float("inf"))
    if isinstance(k, bool) or not isinstance(k, (int, float)) or k != k or k < 1 or (k != float("inf") and k != int(k)):
        raise ValueError(f"targets_config.k must be inf or an integer >= 1, not {k!r}")
    if k >= 2 ** 31:
        k = float("inf")  # (no instance has that many pixels)
    return (L.AFFINITY_BEV if name == "BEV" else L.AFFINITY_GAUSSIAN), normalize, (0 if k == float("inf") else int(k))


def _soft_is_default(soft: Tuple[int, bool, int]) -> bool:
    return soft == (L.AFFINITY_GAUSSIAN, False, 0)


def _stage_annotations(x: Dict[str, Any], B: int, dev: torch.device):
    """Annotation table grouped by sweep -> (cuboids (m,10) f64, CSR offsets (B+1) i32) on the device through ONE pinned staging buffer."""
    cub = annotations_to_cuboids(x["annotations"])
    order = np.argsort(cub[:, -1], kind="stable") if cub.shape[0] else np.zeros(0, dtype=np.int64)
    cub = cub[order]
    counts_per = np.bincount(cub[:, -1].astype(np.int64), minlength=B) if cub.shape[0] else np.zeros(B, dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts_per)]).astype(np.int32)
    m = int(cub.shape[0])
    # ONE pinned staging buffer, uploaded without blocking the host: a pageable `.to(device)` waits until the stream has drained
    # (the whole forward pass, ~20 ms twice per step: the host lost its lead over the GPU right before the backward pass)
    stage = torch.empty(10 * max(m, 1) + (B + 1 + 1) // 2, dtype=torch.float64, pin_memory=True)
    stage[: 10 * m].view(m, 10).copy_(torch.from_numpy(np.ascontiguousarray(cub)))
    stage[10 * max(m, 1) :].view(torch.int32)[: B + 1].copy_(torch.from_numpy(offsets))
    stage_d = stage.to(dev, non_blocking=True)
    return stage_d[: 10 * m].view(m, 10), stage_d[10 * max(m, 1) :].view(torch.int32)[: B + 1], m


def compute_targets(x: Dict[str, Any], tasks_config: Mapping, fpn_strides: Sequence[int], targets_config: Any) -> Dict[int, Dict[int, Dict[str, Tensor]]]:
    """Dense targets per stride / task (``detection_head.py:496-665``) on the device, for any list of strides and tasks.

    Level ``s`` sees the columns ``::s`` of the sweep; with ``fpn_assignment_method == "RANGE"`` an annotation belongs to it iff
    ``lower < ||centre|| <= upper`` of ``range_partitions[s]``.  Boxes are ranked per (sweep, level, task) by their interior-point
    count at the level's resolution.  An annotation belongs to a task by its ``task_id`` column: the reference splits a sweep's rows by
    ``unique(return_counts=True)`` of that column, which is the same thing only for rows sorted by task within a sweep (the loader
    sorts them so); the fixtures feed rows sorted by (sweep, task).  One level of stride 1, one task, no RANGE filter: the one-level
    kernels, which ignore the task column as they always did.
    """
    cart = x["cart"]
    _require_cuda(cart, "cart")
    strides, tasks = [int(s) for s in fpn_strides], list(tasks_config.keys())
    method = _assignment_method(targets_config)
    az_inv = bool(_cfg_get(targets_config, "enable_azimuth_invariant_targets", True))
    B, _, H, W = cart.shape
    dev = cart.device
    cub_d, off_d, m = _stage_annotations(x, B, dev)
    cart32 = cart.detach().float().contiguous()
    result = _assign_targets(cart32, cub_d, off_d, m, tasks_config, strides, tasks, targets_config, method, az_inv)
    if not _soft_is_default(soft_options(targets_config)):
        for level in result.values():  # rv_soft_assign indexes its instance table by the CSR of the annotation table
            for tg in level.values():
                tg["box_offsets"], tg["box_count"] = off_d, m
    return result


def _assign_targets(cart32: Tensor, cub_d: Tensor, off_d: Tensor, m: int, tasks_config: Mapping, strides: Sequence[int],
                         tasks: Sequence[Any], targets_config: Any, method: Optional[str], az_inv: bool):
    B, _, H, W = cart32.shape
    dev = cart32.device
    if strides != [1] or len(tasks) != 1 or method is not None:
        return _compute_targets_multilevel(cart32, cub_d, off_d, m, tasks_config, strides, tasks, targets_config, method, az_inv)
    t_id = tasks[0]
    n_cls = len(tasks_config[t_id])
    scratch = torch.empty((3, max(m, 1)), dtype=torch.int32, device=dev)
    labels = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    pan = torch.empty((B, 1, H, W), dtype=torch.int64, device=dev)
    reg = torch.empty((B, 8, H, W), dtype=torch.float32, device=dev)
    ppo = torch.empty((B, 1, H, W), dtype=torch.int64, device=dev)
    nobj = torch.empty(1, dtype=torch.int32, device=dev)
    L.call("rv_assign_targets", L.ptr(cub_d) if m else None, m, L.ptr(off_d), L.ptr(cart32), B, H, W,
           n_cls, 1 if az_inv else 0, L.ptr(scratch[0]), L.ptr(scratch[1]), L.ptr(scratch[2]), L.ptr(labels),
           L.ptr(pan), L.ptr(reg), L.ptr(ppo), L.ptr(nobj), L.stream_ptr())
    return {1: {t_id: {"points_per_obj": ppo, "panoptics": pan, "classification_labels": labels, "regression_targets": reg,
                       "num_objects": nobj, "num_category": torch.ones((B, n_cls, 1, 1), device=dev)}}}


def _compute_targets_multilevel(cart32: Tensor, cub_d: Tensor, off_d: Tensor, m: int, tasks_config: Mapping, strides: Sequence[int],
                                tasks: Sequence[Any], targets_config: Any, method: Optional[str], az_inv: bool):
    """Every level and task through ``rv_assign_targets_multilevel``: the slab tests once per (full-resolution pixel, box)."""
    B, _, H, W = cart32.shape
    dev = cart32.device
    n_l, n_t = len(strides), len(tasks)
    if n_l > L.ML_MAX_LEVELS or n_l * n_t > L.ML_MAX_ENTRIES:
        raise NotImplementedError(f"{n_l} levels x {n_t} tasks: the kernels take at most {L.ML_MAX_LEVELS} levels and {L.ML_MAX_ENTRIES} (level, task) pairs")
    levels = (L.TargetLevel * n_l)()
    for i, s in enumerate(strides):
        if W % s:
            raise ValueError(f"stride {s} does not divide the sweep width {W}")
        lower, upper = _partition(targets_config, s) if method == "RANGE" else (0.0, float("inf"))
        levels[i] = L.TargetLevel(s, 1 if method == "RANGE" else 0, lower, upper)
    task_ids = (ctypes.c_int32 * n_t)(*[int(t) for t in tasks])
    task_cls = (ctypes.c_int32 * n_t)(*[len(tasks_config[t]) for t in tasks])
    outs = (L.TargetOut * (n_l * n_t))()
    nobj = torch.empty(n_l * n_t, dtype=torch.int32, device=dev)
    scratch = torch.empty(3 * n_l * max(m, 1), dtype=torch.int32, device=dev)
    result: Dict[int, Dict[Any, Dict[str, Tensor]]] = {}
    for i, s in enumerate(strides):
        ws = W // s
        result[s] = {}
        for k, t in enumerate(tasks):
            e = i * n_t + k
            tg = {"points_per_obj": torch.empty((B, 1, H, ws), dtype=torch.int64, device=dev),
                  "panoptics": torch.empty((B, 1, H, ws), dtype=torch.int64, device=dev),
                  "classification_labels": torch.empty((B, H, ws), dtype=torch.int64, device=dev),
                  "regression_targets": torch.empty((B, 8, H, ws), dtype=torch.float32, device=dev),
                  "num_objects": nobj[e : e + 1], "num_category": torch.ones((B, len(tasks_config[t]), 1, 1), device=dev)}
            outs[e] = L.TargetOut(tg["classification_labels"].data_ptr(), tg["panoptics"].data_ptr(), tg["regression_targets"].data_ptr(),
                                  tg["points_per_obj"].data_ptr())
            result[s][t] = tg
    L.call("rv_assign_targets_multilevel", L.ptr(cub_d) if m else None, m, L.ptr(off_d), L.ptr(cart32), B, H, W,
           n_l, levels, n_t, task_ids, task_cls, 1 if az_inv else 0, L.ptr(scratch), outs, L.ptr(nobj), L.stream_ptr())
    return result


def _nhwc_f32(x: Tensor) -> Tuple[Tensor, int]:
    """(N,C,H,W) fp32 tensor -> (storage tensor to keep alive, channel stride) for the NHWC kernels (zero-copy for head outputs)."""
    n, c, h, w = x.shape
    if x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(2) == w * x.stride(3) and x.stride(0) == h * w * x.stride(3):
        return x, x.stride(3)
    y = x.detach().float().permute(0, 2, 3, 1).contiguous()
    return y, c


class _DetectionLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: Tensor, regressands: Tensor, cart: Tensor, mask: Tensor, tg: Dict[str, Tensor], hp: Dict[str, Any]):
        dev = logits.device
        B, n_cls, H, W = logits.shape
        lg, ld_l = _nhwc_f32(logits)
        rg, ld_r = _nhwc_f32(regressands)
        cart32 = cart.detach().float().contiguous()
        mask8 = mask.detach().reshape(B, H, W).to(torch.uint8).contiguous()
        sums = torch.empty(24, dtype=torch.float64, device=dev)
        soft = torch.empty((B, n_cls, H, W), dtype=torch.float32, device=dev)
        fg = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        coding = (ctypes.c_float * 8)(*[float(v) for v in hp["coding_weights"]])
        args = (L.ptr(lg), ld_l, L.ptr(rg), ld_r, L.ptr(cart32), L.ptr(mask8), L.ptr(tg["classification_labels"]),
                L.ptr(tg["panoptics"]), L.ptr(tg["regression_targets"]), L.ptr(tg["points_per_obj"]), L.ptr(tg["num_objects"]),
                B, n_cls, H, W, coding, hp["cls_weight"], hp["reg_weight"],
                hp["smoothing"], hp["sigma"], hp["alpha"], hp["gamma"], 1 if hp["az_inv"] else 0)
        L.call("rv_detection_loss_forward", *args, L.ptr(sums), L.ptr(soft), L.ptr(fg), L.stream_ptr())
        ctx.args, ctx.keep = args, (lg, rg, cart32, mask8, tg, coding)
        ctx.sums, ctx.meta = sums, (B, n_cls, H, W, ld_l, ld_r, logits.dtype, regressands.dtype)
        ctx.mark_non_differentiable(sums, soft, fg)
        loss = sums[16].clone()  # (formed by the kernel: sums[0] / sums[13] + sum(sums[4:12]) / sums[12])
        return loss, sums, soft, fg

    @staticmethod
    def backward(ctx, g_loss, *_):
        B, n_cls, H, W, ld_l, ld_r, dt_l, dt_r = ctx.meta
        dev = ctx.sums.device
        # (padding channels beyond n_cls / 8 are never written and never read: the returned gradients are slices)
        d_l = torch.empty((B, H, W, ld_l), dtype=torch.float32, device=dev)
        d_r = torch.empty((B, H, W, ld_r), dtype=torch.float32, device=dev)
        ctx.sums[15:16].copy_(g_loss.reshape(1))  # the incoming gradient as the kernel's device-side factor: one 8-byte copy instead of two passes over the gradients
        L.call("rv_detection_loss_backward", *ctx.args, L.ptr(ctx.sums), 1.0, L.ptr(d_l), L.ptr(d_r), L.stream_ptr())
        return (d_l[..., :n_cls].permute(0, 3, 1, 2).to(dt_l), d_r[..., :8].permute(0, 3, 1, 2).to(dt_r), None, None, None, None)


# rows of loss sums: where ``loss_finish_kernel`` / ``loss_table_finish_kernel`` leave the scalars of the loss dict
SUMS_INDEX = {"loss": 16, "classification_loss": 17, "foreground_loss": 18, "background_loss": 19, "regression_loss": 23,
              "coordinate_loss": 20, "dimension_loss": 21, "rotation_loss": 22, "total_fg": 13, "total_objects": 12}


class _MultiLevelLossFn(torch.autograd.Function):
    """The loss of every (level, task) entry as ONE node: phase one (one launch over the entry table) and phase two (the global
    normalisers and every reported scalar) in forward, one launch in backward.  ``entries`` is a list of dicts (cart, mask, targets);
    forward adds each entry's soft targets and foreground map to its dict.  Tensor inputs: logits, regressands of entry 0, 1, ...

    ``hp["soft"]`` (``soft_options``; absent = the per-pixel GAUSSIAN affinity inside the loss kernel): forward first runs ``rv_soft_assign``
    over the same entry table -- every entry's affinity map, selected per instance on the device -- and the ``_aff`` loss pair reads the
    maps; backward reuses the maps forward saved (the affinity comes from detached inputs: there is no second selection).

    ``hp["kinds"]`` (``(RV_CLS_*, RV_REG_*, beta / delta)``; absent = varifocal + L1 on the pairs above): the same node on the
    ``rv_detection_loss_table_*`` pair, with the maps when ``hp["soft"]`` asks for them."""

    @staticmethod
    def forward(ctx, entries, hp: Dict[str, Any], *tensors: Tensor):
        n = len(entries)
        dev = tensors[0].device
        width = L.loss_sums_len()
        sums = torch.empty((n + 1, width), dtype=torch.float64, device=dev)
        table = (L.LossEntry * n)()
        keep, meta = [], []
        for e, ent in enumerate(entries):
            logits, regressands = tensors[2 * e], tensors[2 * e + 1]
            B, n_cls, H, W = logits.shape
            lg, ld_l = _nhwc_f32(logits)
            rg, ld_r = _nhwc_f32(regressands)
            cart32 = ent["cart"].detach().float().contiguous()
            mask8 = ent["mask"].detach().reshape(B, H, W).to(torch.uint8).contiguous()
            tg = ent["targets"]
            ent["soft"] = torch.empty((B, n_cls, H, W), dtype=torch.float32, device=dev)
            ent["foreground"] = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
            table[e] = L.LossEntry(lg.data_ptr(), rg.data_ptr(), cart32.data_ptr(), mask8.data_ptr(), tg["classification_labels"].data_ptr(),
                                   tg["panoptics"].data_ptr(), tg["regression_targets"].data_ptr(), tg["points_per_obj"].data_ptr(),
                                   tg["num_objects"].data_ptr(), ent["soft"].data_ptr(), ent["foreground"].data_ptr(), None, None,
                                   ld_l, ld_r, B, n_cls, H, W)
            keep.append((lg, rg, cart32, mask8, tg))
            meta.append((B, n_cls, H, W, ld_l, ld_r, logits.dtype, regressands.dtype))
        params = L.LossParams((ctypes.c_float * 8)(*[float(v) for v in hp["coding_weights"]]), hp["cls_weight"], hp["reg_weight"], hp["smoothing"],
                              hp["sigma"], hp["alpha"], hp["gamma"], 1 if hp["az_inv"] else 0)
        ctx.maps = None
        ctx.kinds = L.LossKinds(*hp["kinds"]) if hp.get("kinds") is not None else None
        if hp.get("soft") is None:
            if ctx.kinds is None:
                L.call("rv_detection_loss_multilevel_forward", table, n, params, L.ptr(sums), L.stream_ptr())
            else:
                L.call("rv_detection_loss_table_forward", table, n, params, ctx.kinds, None, L.ptr(sums), L.stream_ptr())
        else:
            fn, normalize, k = hp["soft"]
            off_d, m = hp["box_offsets"], int(hp["box_count"])
            B = meta[0][0]
            maps = [torch.empty((m_[0], 1, m_[2], m_[3]), dtype=torch.float32, device=dev) for m_ in meta]
            map_ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in maps])
            ws = torch.empty(max(int(L.load().rv_soft_assign_workspace_bytes(n, m, B)), 1), dtype=torch.uint8, device=dev)
            L.call("rv_soft_assign", table, n, params, fn, 1 if normalize else 0, k, L.ptr(off_d),
                   m, L.ptr(ws), map_ptrs, L.stream_ptr())
            if ctx.kinds is None:
                L.call("rv_detection_loss_multilevel_forward_aff", table, n, params, map_ptrs, L.ptr(sums), L.stream_ptr())
            else:
                L.call("rv_detection_loss_table_forward", table, n, params, ctx.kinds, map_ptrs, L.ptr(sums), L.stream_ptr())
            ctx.maps = (map_ptrs, maps)
            for ent, amap in zip(entries, maps):
                ent["affinity"] = amap
        ctx.table, ctx.params, ctx.keep, ctx.meta, ctx.sums = table, params, keep, meta, sums
        ctx.mark_non_differentiable(sums)
        return sums[n, SUMS_INDEX["loss"]].clone(), sums

    @staticmethod
    def backward(ctx, g_loss, *_):
        n, dev = len(ctx.meta), ctx.sums.device
        bufs = []
        for e, (B, n_cls, H, W, ld_l, ld_r, _, _) in enumerate(ctx.meta):
            # (padding channels beyond n_cls / 8 are never written and never read: the returned gradients are slices)
            d_l = torch.empty((B, H, W, ld_l), dtype=torch.float32, device=dev)
            d_r = torch.empty((B, H, W, ld_r), dtype=torch.float32, device=dev)
            ctx.table[e].d_logits, ctx.table[e].d_regressands = d_l.data_ptr(), d_r.data_ptr()
            bufs.append((d_l, d_r))
        ctx.sums[n, 15:16].copy_(g_loss.reshape(1))  # the incoming gradient as the kernel's device-side factor
        if ctx.kinds is not None:
            L.call("rv_detection_loss_table_backward", ctx.table, n, ctx.params, ctx.kinds,
                   None if ctx.maps is None else ctx.maps[0], L.ptr(ctx.sums), 1.0, L.stream_ptr())
        elif ctx.maps is None:
            L.call("rv_detection_loss_multilevel_backward", ctx.table, n, ctx.params, L.ptr(ctx.sums), 1.0, L.stream_ptr())
        else:
            L.call("rv_detection_loss_multilevel_backward_aff", ctx.table, n, ctx.params, ctx.maps[0], L.ptr(ctx.sums), 1.0,
                   L.stream_ptr())
        grads = []
        for (d_l, d_r), (_, n_cls, _, _, _, _, dt_l, dt_r) in zip(bufs, ctx.meta):
            grads += [d_l[..., :n_cls].permute(0, 3, 1, 2).to(dt_l), d_r[..., :8].permute(0, 3, 1, 2).to(dt_r)]
        return (None, None, *grads)


def _instantiate(cfg: Any) -> Any:
    if cfg is None or isinstance(cfg, str):
        return None
    cfg = dict(cfg)
    target = cfg.pop("_target_")
    cfg.pop("_recursive_", None)
    if target.startswith("torchbox3d."):
        target = "range_view_3d_detection_amd." + target[len("torchbox3d."):]
    mod, _, name = target.rpartition(".")
    module = importlib.import_module(mod)
    if not hasattr(module, name):
        raise NotImplementedError(f"{target}: {mod} has no {name}")
    return getattr(module, name)(**cfg)


def _classification_kind(cls_loss: Any) -> Tuple[int, float, float]:
    """``(RV_CLS_* kind, alpha, gamma)`` the fused kernel takes for the instantiated ``_cls_loss`` (``None``: the varifocal defaults).
    The class decides, not its fields: ``FocalLoss`` hands over 0.25 / 2.0 whatever it was configured with (see its docstring)."""
    from ..losses.classification import FocalLoss, PenaltyReducedFocalLoss, VarifocalLoss

    if cls_loss is None:
        return L.CLS_VARIFOCAL, 0.75, 2.0
    if getattr(cls_loss, "reduction", "none") != "none":
        raise NotImplementedError(f"_cls_loss reduction {cls_loss.reduction!r}: the fused loss reduces element-wise losses itself (reduction: none)")
    if type(cls_loss) is VarifocalLoss:
        return L.CLS_VARIFOCAL, float(cls_loss.alpha), float(cls_loss.gamma)
    if type(cls_loss) is FocalLoss:
        return L.CLS_FOCAL, float(cls_loss.kernel_alpha), float(cls_loss.kernel_gamma)
    if type(cls_loss) is PenaltyReducedFocalLoss:
        return L.CLS_PENALTY_REDUCED, float(cls_loss.alpha), float(cls_loss.gamma)
    raise NotImplementedError(f"_cls_loss {type(cls_loss).__module__}.{type(cls_loss).__qualname__}: the fused loss implements VarifocalLoss, "
                              "FocalLoss and PenaltyReducedFocalLoss")


# `_regression_loss._target_` by its exact class name -> (RV_REG_* kind, the keyword of its parameter, torch's default)
_REGRESSION_KINDS = {"L1Loss": (L.REG_L1, None, 0.0), "SmoothL1Loss": (L.REG_SMOOTH_L1, "beta", 1.0), "HuberLoss": (L.REG_HUBER, "delta", 1.0),
                     "MSELoss": (L.REG_MSE, None, 0.0)}


def _regression_kind(cfg: Any) -> Tuple[int, float, nn.Module]:
    """``(RV_REG_* kind, beta / delta, the instantiated torch module)`` of ``_regression_loss`` (``None``: ``torch.nn.L1Loss``).  The target
    is matched by its exact class name under ``torch.nn`` or ``torch.nn.modules.loss`` (a test by suffix once took SmoothL1Loss for L1Loss)."""
    if cfg is None or isinstance(cfg, str):
        return L.REG_L1, 0.0, nn.L1Loss(reduction="none")
    cfg = dict(cfg)
    target = str(cfg.pop("_target_", "torch.nn.L1Loss"))
    cfg.pop("_recursive_", None)
    mod, _, name = target.rpartition(".")
    if mod not in ("torch.nn", "torch.nn.modules.loss") or name not in _REGRESSION_KINDS:
        raise NotImplementedError(f"_regression_loss {target}: the fused loss implements torch.nn.L1Loss, SmoothL1Loss, HuberLoss and MSELoss")
    module = getattr(nn, name)(**cfg)
    if module.reduction != "none":
        raise NotImplementedError(f"_regression_loss reduction {module.reduction!r}: the fused loss reduces element-wise losses itself (reduction: none)")
    kind, key, _ = _REGRESSION_KINDS[name]
    param = float(getattr(module, key)) if key else 0.0
    if (kind == L.REG_SMOOTH_L1 and not param >= 0.0) or (kind == L.REG_HUBER and not param > 0.0) or param == float("inf"):
        raise ValueError(f"_regression_loss {target}: {key} = {param}")
    return kind, param, module


class DetectionHead(nn.Module):
    """Per-stride x per-task classification / regression towers + losses."""

    def __init__(self, fpn: Mapping, fpn_kernel_sizes: Mapping, targets_config: Any, num_classification_blocks: int,
                 num_regression_blocks: int, final_kernel_size: int, tasks_cfg: Mapping, task_in_channels: int,
                 classification_weight: float, regression_weight: float, coding_weights: Sequence[float],
                 classification_head_channels: int, regression_head_channels: int, classification_normalization_method: str,
                 additive_smoothing: float = 1.0, _cls_loss: Any = None, _regression_loss: Any = None, compile: bool = False) -> None:
        super().__init__()
        self.fpn, self.fpn_kernel_sizes, self.targets_config = fpn, fpn_kernel_sizes, targets_config
        self.num_classification_blocks, self.num_regression_blocks = num_classification_blocks, num_regression_blocks
        self.final_kernel_size, self.tasks_cfg, self.task_in_channels = final_kernel_size, tasks_cfg, task_in_channels
        self.classification_weight, self.regression_weight = classification_weight, regression_weight
        self.coding_weights = list(coding_weights)
        self.classification_head_channels, self.regression_head_channels = classification_head_channels, regression_head_channels
        self.classification_normalization_method = classification_normalization_method
        self.additive_smoothing, self.compile = additive_smoothing, compile
        self.classification_head = nn.ModuleDict({
            str(stride): nn.ModuleDict({
                str(k): DenseHead(num_channels, classification_head_channels, len(categories), kernel_size=fpn_kernel_sizes[stride],
                                  final_kernel_size=final_kernel_size, prior_prob=FOCAL_PRIOR_PROB, num_blocks=num_classification_blocks)
                for k, categories in tasks_cfg.items()})
            for stride, num_channels in fpn.items()})
        self.regression_head = nn.ModuleDict({
            str(stride): nn.ModuleDict({
                str(k): DenseHead(num_channels, regression_head_channels, 8, kernel_size=fpn_kernel_sizes[stride],
                                  final_kernel_size=final_kernel_size, num_blocks=num_regression_blocks)
                for k, _ in tasks_cfg.items()})
            for stride, num_channels in fpn.items()})
        self.cls_loss = _instantiate(_cls_loss)
        _classification_kind(self.cls_loss)  # (an unknown class or reduction raises here, not in the first step)
        reg_kind, reg_param, self.regression_loss = _regression_kind(_regression_loss)
        self._reg_kind = (reg_kind, reg_param)

    def forward(self, input: Dict[int, Tensor], data: Dict[Any, Any], return_loss: bool = False):
        multiscale_outputs: Dict[int, Dict[Any, Any]] = {}
        method = _assignment_method(self.targets_config)
        for stride in self.fpn.keys():
            s = int(stride)
            feats = input[s]
            features = data["features"][:, :, ::1, ::s].clone()
            cart = data["cart"][:, :, ::1, ::s].clone()
            mask = data["mask"][:, :, ::1, ::s].clone()
            multiscale_outputs[s] = {"features": features, "cart": cart, "mask": mask}
            if method == "RANGE":  # (:154-158) in place: the loss and the decoder see the partitioned mask
                lower, upper = _partition(self.targets_config, stride)
                dists = torch.linalg.vector_norm(cart, dim=1, keepdim=True)
                mask.mul_((dists > lower) & (dists <= upper))
            # one program (one autograd node) per task: with several tasks at a level autograd adds the tasks' input gradients
            # in len(tasks) - 1 passes of its own over the level's feature gradient
            for task_id in self.tasks_cfg.keys():
                logits, regressands = forward_pair(self.classification_head[str(stride)][str(task_id)],
                                                   self.regression_head[str(stride)][str(task_id)], feats)
                multiscale_outputs[s][task_id] = {"logits": logits, "regressands": regressands}
        losses: Dict[str, Any] = {}
        if return_loss:
            targets = compute_targets(data, tasks_config=self.tasks_cfg, fpn_strides=list(self.fpn.keys()), targets_config=self.targets_config)
            for k, v in targets.items():
                data[k] = v
            losses = self.loss(multiscale_outputs, data)
        return multiscale_outputs, losses

    def loss(self, multiscale_outputs: Dict[int, Dict[Any, Any]], multiscale_data: Dict[Any, Any]) -> Dict[str, Any]:
        """``DetectionHead.loss`` + ``reduce_multiscale_loss`` (``detection_head.py:202-449``).

        Every (level, task) is normalised by ``total_fg`` (foreground pixels of ALL levels and tasks + ``additive_smoothing``) and
        ``total_objects`` (objects of all levels and tasks, at least 1).  The dict holds each scalar summed over the (level, task) list;
        ``total_fg`` / ``total_objects`` are summed over that list too, as the reference does, so they read ``n_entries x`` the value.
        The reference fills ``"{name}/s{stride}"`` from position ``i`` of the stride in a list that has ``levels x tasks`` entries in
        stride-major order: with more than one task ``/s{strides[i]}`` is entry ``i`` of that list, not the level's sum.  Reproduced.
        """
        strides, tasks = [int(s) for s in self.fpn.keys()], list(self.tasks_cfg.keys())
        tc = self.targets_config
        soft = soft_options(tc)
        cls_kind, alpha, gamma = _classification_kind(self.cls_loss)
        hp = {
            "coding_weights": self.coding_weights, "cls_weight": float(self.classification_weight), "reg_weight": float(self.regression_weight),
            "smoothing": float(self.additive_smoothing), "sigma": float(_cfg_get(tc, "sigma", 0.75)),
            "alpha": alpha, "gamma": gamma,
            "az_inv": bool(_cfg_get(tc, "enable_azimuth_invariant_targets", True)),
        }
        if (cls_kind, self._reg_kind[0]) != (L.CLS_VARIFOCAL, L.REG_L1):
            # any other loss kind: the table node on the rv_detection_loss_table_* pair (one entry is a legal table); the default kinds
            # keep the three routes below, launch for launch
            hp["kinds"] = (cls_kind, self._reg_kind[0], self._reg_kind[1])
        if not _soft_is_default(soft):
            # a per-instance affinity (BEV, normalize_affinities, finite k): one entry is a legal table, so the one-level recipe goes
            # through the multi-level node too; the instance table is indexed by the CSR of the annotation table
            tg0 = multiscale_data[strides[0]][tasks[0]]
            if "box_offsets" in tg0:
                hp["box_offsets"], hp["box_count"] = tg0["box_offsets"], tg0["box_count"]
            else:  # (targets that did not come from compute_targets: the same CSR from the annotation table, one small upload)
                out0 = multiscale_outputs[strides[0]]
                _, hp["box_offsets"], hp["box_count"] = _stage_annotations(multiscale_data, out0["cart"].shape[0], out0["cart"].device)
            hp["soft"] = soft
            return self._multilevel_loss(multiscale_outputs, multiscale_data, strides, tasks, hp)
        if "kinds" in hp or strides != [1] or len(tasks) != 1 or _assignment_method(tc) is not None:
            return self._multilevel_loss(multiscale_outputs, multiscale_data, strides, tasks, hp)
        stride, task_id = strides[0], tasks[0]
        out = multiscale_outputs[stride]
        tg = multiscale_data[stride][task_id]
        flat = {"classification_labels": tg["classification_labels"], "panoptics": tg["panoptics"], "regression_targets": tg["regression_targets"],
                "points_per_obj": tg["points_per_obj"], "num_objects": tg["num_objects"]}
        loss, sums, soft, fg = _DetectionLossFn.apply(out[task_id]["logits"], out[task_id]["regressands"], out["cart"], out["mask"], flat, hp)
        tg["targets"] = soft
        # (views of the scalars loss_finish_kernel formed on the device: no launches here)
        task = {name: sums[i] for name, i in SUMS_INDEX.items()}
        task["loss"] = loss
        losses: Dict[str, Any] = dict(task)
        for name, v in task.items():
            losses[f"{name}/s{stride}"] = v
        mask = out["mask"]
        bg = torch.logical_and(fg.logical_not(), mask)
        losses["aux"] = {stride: {task_id: {"targets": soft, "foreground": fg, "background": bg.float(), "mask": mask,
                                            "point_counts": tg["points_per_obj"]}}}
        return losses

    def _multilevel_loss(self, multiscale_outputs: Dict[int, Dict[Any, Any]], multiscale_data: Dict[Any, Any], strides: Sequence[int],
                         tasks: Sequence[Any], hp: Dict[str, Any]) -> Dict[str, Any]:
        entries, tensors = [], []
        for stride in strides:
            out = multiscale_outputs[stride]
            for task_id in tasks:
                entries.append({"stride": stride, "task": task_id, "cart": out["cart"], "mask": out["mask"], "targets": multiscale_data[stride][task_id]})
                tensors += [out[task_id]["logits"], out[task_id]["regressands"]]
        loss, sums = _MultiLevelLossFn.apply(entries, hp, *tensors)
        n = len(entries)
        # (views of the scalars loss_table_finish_kernel formed on the device: no launches here)
        losses: Dict[str, Any] = {name: sums[n, i] for name, i in SUMS_INDEX.items()}
        losses["loss"] = loss
        for name, i in SUMS_INDEX.items():
            for pos, stride in enumerate(strides):  # position in the stride-major (level, task) list, as the reference indexes it
                losses[f"{name}/s{stride}"] = sums[pos, i]
        aux: Dict[int, Dict[Any, Dict[str, Tensor]]] = {}
        for ent in entries:
            tg, mask, fg = ent["targets"], ent["mask"], ent["foreground"]
            tg["targets"] = ent["soft"]
            bg = torch.logical_and(fg.logical_not(), mask)
            aux.setdefault(ent["stride"], {})[ent["task"]] = {"targets": ent["soft"], "foreground": fg, "background": bg.float(), "mask": mask,
                                                             "point_counts": tg["points_per_obj"]}
        losses["aux"] = aux
        return losses
