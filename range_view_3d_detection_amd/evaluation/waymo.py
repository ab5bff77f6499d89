"""Detection evaluation with the Waymo Open Dataset metric definitions, on the device: rotated BEV / 3-D IoU, maximum-weight matching
at the 101 score cutoffs, AP and APH per object type, range and difficulty level.

Replaces ``evaluate_waymo`` as ``Detector.on_validation_end`` calls it (``nn/arch/detector.py:498-516``, ``evaluation/evaluate.py``).
``waymo_open_dataset`` and TensorFlow are not part of the reference tree: the matching and the metric are DECLARED (``include/rv3d.h``,
DESIGN.md 8.3) and not pinned against that library's binaries.  Pinned to the reference: the ground-truth filter and the level rule
(``evaluate.py:325-333``), the object types (``:68``), frames = the sweeps with ground truth (``:382-389``), yaw from the quaternion
(``:269-286``, rounded to fp32 with the box ``:407-408``), the configuration (``:289-319``) and the result layout (``:70-243``).

The three steps (``rv_waymo_iou``, ``rv_waymo_match``, ``rv_waymo_summarize``) are HIP kernels; torch orders the rows (:mod:`.rows`: one stable
``sort`` per side, segment offsets by ``searchsorted``).  ``update`` reads nothing back and keeps only the integer count tables
(2 x 16 x 2 x 101 x 4 int64) between steps.  No CPU fallback.
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Mapping, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from ..engine import _require_cuda
from ..math.ops.coding import _column
from .rows import ClassMap, frame_rows, order_rows, stray_rows_message, sweep_index, task_bases

OBJECT_TYPES = {"VEHICLE": 1, "PEDESTRIAN": 2, "SIGN": 3, "CYCLIST": 4}  # evaluate.py:68
RANGE_SHARDS = ((0.0, math.inf), (0.0, 30.0), (30.0, 50.0), (50.0, math.inf))  # shard 0 = all ranges
BOX_TYPES = ("BEV", "3D")
LEVELS = (1, 2)
RESULT_COLUMNS = ("metric_name", "type", "category", "level", "r_lower", "r_upper", "value")
TABLE_SHAPE = (2, L.WAYMO_NUM_BREAKDOWN_ROWS, 2, L.WAYMO_NUM_CUTOFFS, 4)
_ERRORS = (f"(sweep, type) segments with more than {L.WAYMO_MAX_DTS} detections (RV_WAYMO_MAX_DTS)",
           f"(sweep, type) segments with more than {L.WAYMO_MAX_GTS} ground-truth boxes (RV_WAYMO_MAX_GTS)",
           "segments whose pair offsets do not fit the workspace", "searches that hit their iteration bound")


@dataclass(frozen=True)
class WaymoDetectionCfg:
    """``build_config`` (``evaluate.py:289-319``): IoU thresholds by object type (index 0 is unused); the breakdowns (OBJECT_TYPE and
    RANGE at LEVEL_1 / LEVEL_2), the Hungarian matcher, both box types and the 101 score cutoffs are fixed."""

    iou_thresholds: Tuple[float, ...] = (0.0, 0.7, 0.5, 0.5, 0.5)


def result_layout() -> List[Tuple[str, str, str, int, float, float]]:
    """``(metric_name, type, category, level, r_lower, r_upper)`` of the 128 result rows: the 64 ``AP`` rows of the reference's frame
    (``BEV`` then ``3D``; per type the 4 categories x 2 levels over all ranges, then per category the 3 ranges x 2 levels), then the 64
    ``APH`` rows in the same order."""
    rows = []
    for metric in ("AP", "APH"):
        for box in BOX_TYPES:
            rows += [(metric, box, cat, lvl) + RANGE_SHARDS[0] for cat in OBJECT_TYPES for lvl in LEVELS]
            rows += [(metric, box, cat, lvl) + rng for cat in OBJECT_TYPES for rng in RANGE_SHARDS[1:] for lvl in LEVELS]
    return rows


def difficulty_levels(num_interior_pts: Tensor, difficulty_level: Optional[Tensor] = None) -> Tensor:
    """Level of every ground-truth row, uint8: 0 = dropped (``num_interior_pts <= 0``); else its ``difficulty_level`` when non-zero,
    else 2 with at most 5 interior points, else 1 (``evaluate.py:325-333``)."""
    npts = num_interior_pts.reshape(-1).to(torch.int64)
    level = torch.where(npts <= 5, 2, 1)
    if difficulty_level is not None:
        given = difficulty_level.reshape(-1).to(npts.device).to(torch.int64)
        level = torch.where(given != 0, given, level)
    return torch.where(npts > 0, level, 0).clamp(0, 255).to(torch.uint8)


def boxes_from_rows(rows: Tensor) -> Tensor:
    """(n, 10) fp32 rows in ``DETECTION_COLUMNS`` order -> (n, 7) fp32 ``[x, y, z, l, w, h, yaw]``: yaw in fp64 from the fp32
    quaternion (``quat_to_yaw``), rounded to fp32 with the box."""
    r = rows.float().double()
    qw, qx, qy, qz = r[:, 6], r[:, 7], r[:, 8], r[:, 9]
    yaw = torch.atan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz))
    return torch.cat([r[:, :6], yaw[:, None]], 1).float().contiguous()


def _workspace_views(ws: Tensor, n_segments: int) -> Tuple[Tensor, Tensor]:
    """(pair offsets (n_segments + 1,) i64, IoU table (pairs, 2) f32) of an ``rv_waymo_iou`` workspace (layout: ``include/rv3d.h``)."""
    head = ((n_segments + 1) * 8 + 255) & ~255
    return ws[:n_segments + 1], ws[head // 8:].view(torch.float32).view(-1, 2)


def pairwise_iou(dts: Tensor, dt_order: Tensor, dt_off: Tensor, gts: Tensor, gt_order: Tensor, gt_off: Tensor, n_segments: int) -> Tensor:
    """``rv_waymo_iou``: the workspace (int64 words) holding the pair offsets and the (BEV, 3-D) IoU of every pair of a segment."""
    _require_cuda(dts, "detections")
    _require_cuda(gts, "ground truth")
    n, m = dts.shape[0], gts.shape[0]
    ws_bytes = L.load().rv_waymo_match_workspace_bytes(n, m, n_segments)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dts.device)
    L.call("rv_waymo_iou", L.ptr(dts), L.ptr(dt_order), L.ptr(dt_off), n, L.ptr(gts), L.ptr(gt_order), L.ptr(gt_off), m,
           n_segments, L.ptr(ws), L.stream_ptr())
    return ws


def accumulate(dts: Tensor, scores: Tensor, dt_segment: Tensor, gts: Tensor, gt_level: Tensor, gt_segment: Tensor, n_sweeps: int,
               cfg: WaymoDetectionCfg, tables: Tensor, errors: Tensor, sweep_valid: Optional[Tensor] = None) -> Tensor:
    """One step into ``tables`` / ``errors``: boxes (N,7) / (M,7) f32, ``scores`` (N,) f32, segments int64 (``sweep * 4 + type - 1``;
    ``4 * n_sweeps`` = no segment), ``gt_level`` (M,) u8.  ``sweep_valid`` defaults to "the sweep has ground truth of level != 0".
    Asynchronous on the current stream; returns the IoU workspace (the tests read it)."""
    _require_cuda(dts, "detections")
    _require_cuda(gts, "ground truth")
    dev, n, m, n_seg = dts.device, dts.shape[0], gts.shape[0], 4 * n_sweeps
    if len(cfg.iou_thresholds) != 5:
        raise L.RvError(f"{len(cfg.iou_thresholds)} IoU thresholds (5: index 0 unused, then VEHICLE, PEDESTRIAN, SIGN, CYCLIST)")
    dt_order, dt_off, gt_order, gt_off = order_rows(dt_segment, scores, gt_segment, n_seg)
    if sweep_valid is None:
        inside = (gt_segment >= 0) & (gt_segment < n_seg) & (gt_level != 0)
        sweep_valid = torch.zeros(n_sweeps + 1, dtype=torch.int64, device=dev).index_add_(
            0, torch.where(inside, gt_segment >> 2, n_sweeps), inside.to(torch.int64))
        sweep_valid = (sweep_valid[:n_sweeps] > 0).to(torch.uint8)
    ws = pairwise_iou(dts, dt_order, dt_off, gts, gt_order, gt_off, n_seg)
    thresholds = (ctypes.c_float * 5)(*[float(t) for t in cfg.iou_thresholds])
    L.call("rv_waymo_match", L.ptr(dts), L.ptr(scores), L.ptr(dt_order), L.ptr(dt_off), n, L.ptr(gts), L.ptr(gt_level),
           L.ptr(gt_order), L.ptr(gt_off), m, L.ptr(sweep_valid), n_sweeps, thresholds, L.ptr(ws), L.ptr(tables),
           L.ptr(errors), L.stream_ptr())
    return ws


def summarize(tables: Tensor) -> Tensor:
    """``rv_waymo_summarize``: (2, 16, 2, 101, 4) int64 counts -> (2, 32, 2) f64 (box type, result row, [AP, APH]) on the device."""
    _require_cuda(tables, "tables")
    out = torch.empty((2, L.WAYMO_NUM_RESULT_ROWS, 2), dtype=torch.float64, device=tables.device)
    L.call("rv_waymo_summarize", L.ptr(tables.contiguous()), L.ptr(out), L.stream_ptr())
    return out


def _result_table(values: Tensor):
    """Arrow table ``RESULT_COLUMNS`` from the (2, 32, 2) values: AP rows first, then APH."""
    import pyarrow as pa

    layout = result_layout()
    v = values.cpu()
    column = torch.cat([v[:, :, 0].reshape(-1), v[:, :, 1].reshape(-1)]).numpy()
    cols = {"metric_name": pa.array([r[0] for r in layout], type=pa.string()), "type": pa.array([r[1] for r in layout], type=pa.string()),
            "category": pa.array([r[2] for r in layout], type=pa.string()), "level": pa.array([r[3] for r in layout], type=pa.int64()),
            "r_lower": pa.array([r[4] for r in layout], type=pa.float64()), "r_upper": pa.array([r[5] for r in layout], type=pa.float64()),
            "value": pa.array(column, type=pa.float64())}
    return pa.table(cols)


def _raise_on_errors(errors: Sequence[int], stray: int, max_sweeps: int) -> None:
    if stray:
        raise L.RvError(stray_rows_message(stray, max_sweeps))
    for count, what in zip(errors, _ERRORS):
        if count:
            raise L.RvError(f"{count} {what}: nothing is truncated, the metric is not computed")


class WaymoDetectionEvaluator:
    """Accumulates the Waymo count tables on the device, step by step, and reduces them to AP / APH at the end.

    ``idx_to_category`` lists the category names in class-index order (a list, or the task frame with ``category`` [+ ``task_id``,
    ``offset``] columns), ``tasks`` the head's task table when there are several tasks and no frame; every name must be one of
    ``OBJECT_TYPES`` (the reference's ``replace_strict``).  ``max_sweeps`` bounds ``batch_index`` in an ``update``.

    Stray rows: a detection or annotation whose ``batch_index`` is outside ``[0, n_sweeps)``, or whose class index or task is not in
    the table, is counted on the device and ``compute`` raises (every class here is an object type, so nothing is dropped quietly; the
    AV2 evaluator drops rows of classes it does not evaluate).  ``compute`` also raises for a (sweep, type) with more rows than
    ``RV_WAYMO_MAX_DTS`` / ``RV_WAYMO_MAX_GTS``.
    """

    def __init__(self, cfg: Optional[WaymoDetectionCfg] = None, idx_to_category=tuple(OBJECT_TYPES), tasks: Optional[Mapping[int, Sequence[str]]] = None,
                 max_sweeps: int = 64) -> None:
        self.cfg = cfg or WaymoDetectionCfg()
        names, bases = task_bases(idx_to_category, tasks)
        unknown = [n for n in names if n not in OBJECT_TYPES]
        if unknown:
            raise L.RvError(f"categories {unknown} are not Waymo object types {tuple(OBJECT_TYPES)}")
        # (configuration, not state: kept over reset(), whose next update stays free of copies)
        self._classes = ClassMap([OBJECT_TYPES[n] - 1 for n in names], bases)
        if not 1 <= int(max_sweeps) <= L.WAYMO_MAX_SWEEPS:
            raise L.RvError(f"max_sweeps = {max_sweeps} (1 .. {L.WAYMO_MAX_SWEEPS})")
        self.max_sweeps = int(max_sweeps)
        self.reset()

    def reset(self) -> None:
        self._tables: Optional[Tensor] = None
        self._errors: Optional[Tensor] = None
        self._stray: Optional[Tensor] = None

    def _state(self, dev) -> None:
        if self._tables is None:
            self._tables = torch.zeros(TABLE_SHAPE, dtype=torch.int64, device=dev)
            self._errors = torch.zeros(4, dtype=torch.int32, device=dev)
            self._stray = torch.zeros((), dtype=torch.int64, device=dev)

    def update(self, params: Tensor, scores: Tensor, categories: Tensor, batch_index: Tensor, annotations: Tensor,
               num_interior_pts: Tensor, difficulty_level: Optional[Tensor] = None, n_sweeps: Optional[int] = None) -> None:
        """One validation step: what ``RangeDecoder.decode`` returned -- ``params`` (N,10), ``scores`` (N,), ``categories`` (N,) and
        ``batch_index`` (N,), floats or integers -- and the step's (M,13) annotation rows (``prototype.loader.COLS``: box, ``task_id``,
        ``offset``, ``batch_index``) with their ``num_interior_pts`` (M,) and, where the dataset has it, ``difficulty_level`` (M,).
        ``n_sweeps``: the step's batch size when it is not ``max_sweeps``.  A sweep without ground truth left after the
        ``num_interior_pts > 0`` filter is not a frame: its detections are not evaluated.  Nothing is read back."""
        for t, what in ((params, "params"), (scores, "scores"), (categories, "categories"), (batch_index, "batch_index")):
            _require_cuda(t, what)
        dev = params.device
        n_sweeps = self.max_sweeps if n_sweeps is None else int(n_sweeps)
        if not 1 <= n_sweeps <= L.WAYMO_MAX_SWEEPS:
            raise L.RvError(f"n_sweeps = {n_sweeps} (1 .. {L.WAYMO_MAX_SWEEPS})")
        dt, sc, gt = self._classes.step_rows(params, scores, categories, batch_index, annotations, n_sweeps, 4)
        stray = (~(dt.inside & dt.known)).sum() + (~(gt.inside & gt.known)).sum()  # the Waymo rule: sweep and class (the class docstring)
        level = difficulty_levels(num_interior_pts.detach().to(dev), None if difficulty_level is None else difficulty_level.detach().to(dev))
        self._state(dev)
        accumulate(boxes_from_rows(dt.rows), sc, dt.segment, boxes_from_rows(gt.rows), level, gt.segment, n_sweeps, self.cfg, self._tables,
                   self._errors)
        self._stray += stray

    def tables(self) -> Tensor:
        """The (2, 16, 2, 101, 4) int64 counts seen since ``reset``, summed over the ranks under ``torch.distributed``; raises for rows
        that could not be evaluated."""
        import torch.distributed as dist

        if self._tables is None:
            raise L.RvError("WaymoDetectionEvaluator.compute() before any update()")
        tables = self._tables
        side = torch.cat([self._errors.to(torch.int64), self._stray.reshape(1)])
        if dist.is_available() and dist.is_initialized():
            tables = tables.clone()
            dist.all_reduce(tables)  # (integer sums: exact, whatever the order)
            dist.all_reduce(side)
        side = side.tolist()
        _raise_on_errors(side[:4], side[4], self.max_sweeps)
        return tables

    def compute(self):
        """The metric of everything seen since ``reset`` (every rank's, under ``torch.distributed``): an Arrow table with the columns
        ``RESULT_COLUMNS`` -- the reference frame's 64 ``AP`` rows in its order (``value`` in [0, 1]), then the 64 ``APH`` rows."""
        return _result_table(summarize(self.tables()))

    def summary(self, categories: Sequence[str], table=None) -> List[Tuple[str, str, str, int, float, float, float]]:
        """What ``detector.py:500-503`` logs: value x 100 rounded to 3 digits, level 1, the configured ``categories``, sorted by
        category (stable); one tuple per row, ``RESULT_COLUMNS`` order."""
        table = self.compute() if table is None else table
        rows = zip(*[table.column(c).to_pylist() for c in RESULT_COLUMNS])
        keep = [r[:6] + (round(r[6] * 100.0, 3),) for r in rows if r[3] == 1 and r[2] in set(categories)]
        return sorted(keep, key=lambda r: r[2])


def evaluate_waymo(dts, gts, device: Any = "cuda", cfg: Optional[WaymoDetectionCfg] = None, sweeps_per_call: int = 256):
    """The offline form, mirroring ``evaluate_waymo(dts, gts)`` (``evaluate.py:367``): ``dts`` is what ``write_detections`` wrote,
    concatenated (``DETECTION_COLUMNS``, ``score``, ``log_id``, ``timestamp_ns``, ``category``), ``gts`` has the ``annotations.feather``
    schema (``DETECTION_COLUMNS``, ``category``, ``num_interior_pts``, ``log_id``, ``timestamp_ns`` and, when the dataset has it,
    ``difficulty_level``).  Frames are the (``log_id``, ``timestamp_ns``) groups of the ground truth left after the
    ``num_interior_pts > 0`` filter; detections of any other sweep are dropped.  Returns the table of
    ``WaymoDetectionEvaluator.compute``."""
    import numpy as np

    cfg = cfg or WaymoDetectionCfg()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.RvError(f"evaluate_waymo() on {dev}: the evaluation kernels only run on an MI355X (no CPU fallback)")

    def types_of(frame) -> np.ndarray:
        names = [str(c) for c in _column(frame, "category")]
        unknown = sorted(set(names) - set(OBJECT_TYPES))
        if unknown:
            raise L.RvError(f"categories {unknown} are not Waymo object types {tuple(OBJECT_TYPES)}")
        return np.asarray([OBJECT_TYPES[c] for c in names], dtype=np.int64)

    gt_type, dt_type = types_of(gts), types_of(dts)
    npts = np.asarray(_column(gts, "num_interior_pts"), dtype=np.int64)
    given = np.asarray(_column(gts, "difficulty_level"), dtype=np.int64) if "difficulty_level" in gts.column_names else np.zeros_like(npts)
    frames: Dict[Tuple[str, int], int] = {}
    gt_sweep = sweep_index(gts, frames, keep=npts > 0)
    dt_sweep = sweep_index(dts, frames, add=False)
    dt_rows, gt_rows = frame_rows(dts), frame_rows(gts)
    score = np.asarray(_column(dts, "score"), dtype=np.float32)
    tables = torch.zeros(TABLE_SHAPE, dtype=torch.int64, device=dev)
    errors = torch.zeros(4, dtype=torch.int32, device=dev)
    for first in range(0, max(len(frames), 1), sweeps_per_call):
        n_sweeps = max(min(sweeps_per_call, len(frames) - first), 1)
        d = np.flatnonzero((dt_sweep >= first) & (dt_sweep < first + n_sweeps))
        g = np.flatnonzero((gt_sweep >= first) & (gt_sweep < first + n_sweeps))
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        level = difficulty_levels(to(npts[g]), to(given[g]))
        accumulate(boxes_from_rows(to(dt_rows[d])), to(score[d]), to((dt_sweep[d] - first) * 4 + dt_type[d] - 1),
                   boxes_from_rows(to(gt_rows[g])), level, to((gt_sweep[g] - first) * 4 + gt_type[g] - 1), n_sweeps, cfg, tables, errors)
    _raise_on_errors(errors.tolist(), 0, 0)
    return _result_table(summarize(tables))
