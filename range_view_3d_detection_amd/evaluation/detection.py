"""Detection evaluation on the device: matching, AP, ATE / ASE / AOE, CDS with the AV2 sensor-dataset metric definitions.

Replaces ``prepare_for_evaluation`` + av2's ``evaluate`` as ``Detector.on_validation_end`` calls them
(``nn/arch/detector.py:457-479``).  av2 is not part of the reference tree: the semantics are DECLARED (``include/rv3d.h``)
-- they restate the published AV2 detection metric and are not pinned against av2's binaries.  Pinned to the reference:
``max_range_m`` 150 / inf / 55 (``datasets/__init__.py:27-39``), the detections' range filter on the centre norm
(``detector.py:573-584``), the ground-truth filter ``num_interior_pts > 0`` and ASE's IoU (``math/ops/iou.py:50-55``).

Map-based ROI filtering (``eval_only_roi_instances``, ``datasets/__init__.py:29``: on for AV2 in the reference) runs on the device
too: with ``DetectionCfg.eval_only_roi_instances`` the evaluator takes a ``converters.av2.roi.RoiAtlas`` and, per
sweep, the log's layer and ``city_SE3_ego``; boxes are flagged by ``rv_roi_boxes`` and filtered in ``rv_eval_match_roi``.  Without
the flag (the default) every row handed in counts, subject to the two filters above.

Matching (``rv_eval_match``) and the summary (``rv_eval_summarize``) are HIP kernels; torch orders the rows (:mod:`.rows`: one ``sort`` on a
combined integer key, segment offsets by ``searchsorted``: fixed output sizes, no host synchronisation).  No CPU fallback.
"""

from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from ..engine import _require_cuda
from ..math.ops.coding import _column
from .rows import ClassMap, frame_rows, order_rows, segment_offsets, sort_key, stray_rows_message, sweep_index, task_bases

METRIC_COLUMNS = ("AP", "ATE", "ASE", "AOE", "CDS")
AVERAGE_ROW = "AVERAGE_METRICS"


@dataclass(frozen=True)
class DetectionCfg:
    """av2's ``DetectionCfg``, the fields the metric reads (defaults as there)."""

    categories: Tuple[str, ...] = ()
    affinity_thresholds_m: Tuple[float, ...] = (0.5, 1.0, 2.0, 4.0)
    tp_threshold_m: float = 2.0
    max_range_m: float = 150.0
    max_num_dts_per_category: int = 100
    num_recall_samples: int = 100
    eval_only_roi_instances: bool = False

    @property
    def metrics_defaults(self) -> Tuple[float, float, float]:
        """(ATE, ASE, AOE) of a category without true positives."""
        return (self.tp_threshold_m, 1.0, math.pi)


def detection_cfg_factory(dataset_name: str, valid_categories: Sequence[str], eval_only_roi_instances: Optional[bool] = None) -> DetectionCfg:
    """``datasets/__init__.py:27-48``: ``max_range_m`` 150 (av2), inf (waymo), 55 (nuscenes); categories sorted.
    ``eval_only_roi_instances``: ``None`` keeps the filter off; ``True`` is what the reference sets for AV2
    (``datasets/__init__.py:29``) and needs the evaluator's ``atlas`` / ``roi`` arguments; the reference sets False for waymo and
    nuscenes (``:36, 45``), which have no ROI raster, so ``True`` raises there."""
    name = dataset_name.upper()
    if name == "AV2":
        max_range_m = 150.0
    elif name == "WAYMO":
        max_range_m = math.inf
    elif "NUSCENES" in name:
        max_range_m = 55.0
    else:
        raise L.RvError(f"unknown dataset {dataset_name!r} (av2, waymo, nuscenes)")
    if eval_only_roi_instances and name != "AV2":
        raise L.RvError(f"eval_only_roi_instances=True for {dataset_name!r}: only AV2 has a ROI raster (the reference sets False elsewhere)")
    return DetectionCfg(categories=tuple(sorted(set(valid_categories))), max_range_m=max_range_m,
                        eval_only_roi_instances=bool(eval_only_roi_instances))


def _check_cfg(cfg: DetectionCfg) -> None:
    if not 1 <= len(cfg.affinity_thresholds_m) <= L.EVAL_MAX_THRESHOLDS:
        raise L.RvError(f"{len(cfg.affinity_thresholds_m)} affinity thresholds (1 .. {L.EVAL_MAX_THRESHOLDS})")
    if not 1 <= cfg.max_num_dts_per_category <= L.EVAL_MAX_DTS:
        raise L.RvError(f"max_num_dts_per_category = {cfg.max_num_dts_per_category} (1 .. {L.EVAL_MAX_DTS})")
    if not cfg.categories:
        raise L.RvError("DetectionCfg.categories is empty")


def _check_roi(cfg: DetectionCfg, what: str, *inputs) -> None:
    """The filter and what it needs go together: the flag without its inputs would silently evaluate every box, the inputs without the
    flag would silently be ignored."""
    if cfg.eval_only_roi_instances and any(x is None for x in inputs):
        raise L.RvError(f"cfg.eval_only_roi_instances is set but no {what} was given: the ROI filter needs the logs' rasters (atlas) and "
                        "every sweep's layer and city_SE3_ego")
    if not cfg.eval_only_roi_instances and any(x is not None for x in inputs):
        raise L.RvError(f"{what} given while cfg.eval_only_roi_instances is False: set the flag (detection_cfg_factory('av2', ..., "
                        "eval_only_roi_instances=True)) or drop the argument")


def match(dts: Tensor, scores: Tensor, dt_segment: Tensor, gts: Tensor, gt_valid: Optional[Tensor], gt_segment: Tensor, n_segments: int,
          cfg: DetectionCfg, dt_roi: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """``rv_eval_match`` over rows already labelled with their (sweep, category) segment (``n_segments`` = no segment); with ``dt_roi``
    (N,) uint8, ``rv_eval_match_roi``: a row in range holds its place under the cap whatever its flag, and is evaluated only with a
    non-zero flag (the ground truth's flag goes into ``gt_valid``).

    ``dts`` (N,10) / ``gts`` (M,10) f32 rows in ``DETECTION_COLUMNS`` order, ``scores`` (N,), segments int64, ``gt_valid`` (M,)
    uint8 or None.  Returns ``evaluated`` (N,) u8, ``tp`` (N,T) u8, ``err`` (N,3) f32, ``matched_gt`` (N,) i32 and
    ``gt_evaluated`` (M,) u8, all in input row order.  Asynchronous on the current stream."""
    _require_cuda(dts, "detections")
    _require_cuda(gts, "ground truth")
    dev, n, m, n_thr = dts.device, dts.shape[0], gts.shape[0], len(cfg.affinity_thresholds_m)
    dt_order, dt_off, gt_order, gt_off = order_rows(dt_segment, scores, gt_segment, n_segments)
    out = {"evaluated": torch.empty(n, dtype=torch.uint8, device=dev), "tp": torch.empty((n, n_thr), dtype=torch.uint8, device=dev),
           "err": torch.empty((n, 3), dtype=torch.float32, device=dev), "matched_gt": torch.empty(n, dtype=torch.int32, device=dev),
           "gt_evaluated": torch.empty(m, dtype=torch.uint8, device=dev)}
    thresholds = (ctypes.c_double * n_thr)(*[float(t) for t in cfg.affinity_thresholds_m])
    if dt_roi is not None:
        if dt_roi.dtype != torch.uint8 or dt_roi.device != dev or tuple(dt_roi.shape) != (n,) or not dt_roi.is_contiguous():
            raise L.RvError(f"dt_roi must be {n} contiguous uint8 flags on {dev}")
        roi_arg = (ctypes.c_void_p(dt_roi.data_ptr()),)  # (an empty tensor has no pointer: the kernel reads no flag of 0 rows)
    else:
        roi_arg = ()
    L.call("rv_eval_match" if dt_roi is None else "rv_eval_match_roi", L.ptr(dts), L.ptr(dt_order), L.ptr(dt_off), n, L.ptr(gts),
           L.ptr(gt_valid), L.ptr(gt_order), L.ptr(gt_off), m, n_segments, thresholds, n_thr, cfg.tp_threshold_m,
           cfg.max_range_m, cfg.max_num_dts_per_category, *roi_arg, L.ptr(out["evaluated"]), L.ptr(out["tp"]), L.ptr(out["err"]),
           L.ptr(out["matched_gt"]), L.ptr(out["gt_evaluated"]), L.stream_ptr())
    return out


def summarize(scores: Tensor, categories: Tensor, evaluated: Tensor, tp: Tensor, err: Tensor, n_gt: Tensor,
              cfg: DetectionCfg) -> Tuple[Tensor, Tensor, Tensor]:
    """``rv_eval_summarize`` over the rows of all sweeps, in accumulation order: one sort by (evaluated first, category, score
    descending), the kernel, and the results on the host: table (C + 1, 5) f64 ``METRIC_COLUMNS`` (last row: column means),
    AP per threshold (C, T) f64, evaluated detections per category (C,) i64.  Reads the evaluated-row count back (one
    synchronisation) to size the workspace."""
    _require_cuda(scores, "scores")
    dev, n_cat, n_thr = scores.device, len(cfg.categories), len(cfg.affinity_thresholds_m)
    segment = torch.where(evaluated != 0, categories.to(torch.int64), n_cat)  # rows that were not evaluated: behind every category
    sorted_keys, order = torch.sort(sort_key(segment, scores), stable=True)
    cat_off = segment_offsets(sorted_keys, n_cat, 32)
    offsets = cat_off.cpu()
    n_rows = int(offsets[n_cat])
    order = order[:n_rows]
    flags, errors = tp[order].contiguous(), err[order].contiguous()
    ws_bytes = L.load().rv_eval_summarize_workspace_bytes(n_rows, n_cat, n_thr)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    table = torch.empty((n_cat + 1, 5), dtype=torch.float64, device=dev)
    ap_t = torch.empty((n_cat, n_thr), dtype=torch.float64, device=dev)
    defaults = cfg.metrics_defaults
    L.call("rv_eval_summarize", L.ptr(flags), L.ptr(errors), L.ptr(cat_off), L.ptr(n_gt), n_rows, n_cat, n_thr,
           cfg.tp_threshold_m, cfg.num_recall_samples, defaults[1], defaults[2], L.ptr(ws), L.ptr(table),
           L.ptr(ap_t), L.stream_ptr())
    return table.cpu(), ap_t.cpu(), offsets[1:] - offsets[:-1]


def _metrics_table(cfg: DetectionCfg, table: Tensor, n_dts: Tensor, n_gts: Tensor):
    """Arrow table ``category, AP, ATE, ASE, AOE, CDS, n_dts, n_gts`` (the two counts as ``format_evaluation_metrics`` joins them,
    ``detector.py:651-687``; here: EVALUATED detections and ground truth), ``AVERAGE_METRICS`` last with the totals."""
    import pyarrow as pa

    cols = {"category": pa.array(list(cfg.categories) + [AVERAGE_ROW], type=pa.string())}
    for j, name in enumerate(METRIC_COLUMNS):
        cols[name] = pa.array(table[:, j].contiguous().numpy(), type=pa.float64())
    cols["n_dts"] = pa.array(n_dts.tolist() + [int(n_dts.sum())], type=pa.int64())
    cols["n_gts"] = pa.array(n_gts.tolist() + [int(n_gts.sum())], type=pa.int64())
    return pa.table(cols)


class DetectionEvaluator:
    """Accumulates matched detections on the device, step by step, and reduces them to the metric table at the end.

    ``cfg.categories`` are evaluated (the table's rows, in that order); ``idx_to_category`` lists the category names in
    class-index order (a list, or the task frame with ``category`` [+ ``task_id``, ``offset``] columns), ``tasks`` the head's task
    table when there are several tasks and no frame.  ``max_sweeps`` bounds ``batch_index`` in an ``update`` (the launch grid has to be
    known on the host).  ``atlas``: the ROI rasters of the logs (``converters.av2.roi.RoiAtlas``), required exactly when
    ``cfg.eval_only_roi_instances`` is set.

    Stray rows: a detection or annotation whose ``batch_index`` is outside ``[0, n_sweeps)`` is counted on the device and ``compute``
    raises.  A row of a class that is not in ``cfg.categories``, of an unknown class index or of an unknown task is dropped quietly:
    it has no segment and is never evaluated (the Waymo evaluator raises for those too).
    """

    def __init__(self, cfg: DetectionCfg, idx_to_category, tasks: Optional[Mapping[int, Sequence[str]]] = None, max_sweeps: int = 64,
                 atlas=None) -> None:
        _check_cfg(cfg)
        _check_roi(cfg, "atlas", atlas)
        self.cfg = cfg
        self.atlas = atlas
        names, bases = task_bases(idx_to_category, tasks)
        # class index -> row of cfg.categories, or -1: a class that is not evaluated
        self._classes = ClassMap([cfg.categories.index(n) if n in cfg.categories else -1 for n in names], bases)
        self.max_sweeps = int(max_sweeps)
        self.reset()

    def reset(self) -> None:
        self._n = 0
        self._buf: Dict[str, Tensor] = {}
        self._n_gt: Optional[Tensor] = None
        self._stray: Optional[Tensor] = None

    def _append(self, rows: Dict[str, Tensor]) -> None:
        n = next(iter(rows.values())).shape[0]
        for name, t in rows.items():
            buf = self._buf.get(name)
            if buf is None or self._n + n > buf.shape[0]:
                grown = torch.empty((max(2 * (self._n + n), 4096),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
                if buf is not None:
                    grown[:self._n].copy_(buf[:self._n])
                buf = self._buf[name] = grown
            buf[self._n:self._n + n].copy_(t)
        self._n += n

    def update(self, params: Tensor, scores: Tensor, categories: Tensor, batch_index: Tensor, annotations: Tensor,
               num_interior_pts: Optional[Tensor] = None, n_sweeps: Optional[int] = None, roi: Optional[Tuple[Any, Any]] = None) -> None:
        """One validation step: what ``RangeDecoder.decode`` returned -- ``params`` (N,10), ``scores`` (N,), ``categories`` (N,) and
        ``batch_index`` (N,), floats or integers -- and the step's (M,13) annotation rows (``prototype.loader.COLS``: box, ``task_id``,
        ``offset``, ``batch_index``); ``num_interior_pts`` (M,) when the rows were not filtered yet.  ``n_sweeps``: the step's batch
        size when it is not ``max_sweeps`` (with ``roi``: the length of its sweep table).  Everything stays on the device and
        nothing is read back: one ``rv_eval_match`` on the current stream, the rows of ALL detections appended to the accumulators (compacting to the evaluated ones would need
        a synchronisation).  ``roi`` = (``layer_index`` (B,), ``city_SE3_ego`` (B, 3, 4)) of the step's sweeps, with
        ``cfg.eval_only_roi_instances``: two ``rv_roi_boxes`` launches flag detections and annotations, the annotations' flag is ANDed
        into their validity, and the match is ``rv_eval_match_roi``; still nothing is read back."""
        _check_roi(self.cfg, "roi", roi)
        for t, what in ((params, "params"), (scores, "scores"), (categories, "categories"), (batch_index, "batch_index")):
            _require_cuda(t, what)
        dev, n_cat = params.device, len(self.cfg.categories)
        if roi is not None:  # the sweep table says how many sweeps the step has
            n_roi = int(torch.as_tensor(roi[0]).numel())
            if n_sweeps is not None and int(n_sweeps) != n_roi:
                raise L.RvError(f"roi describes {n_roi} sweeps, n_sweeps = {n_sweeps}")
            n_sweeps = n_roi
        n_sweeps = self.max_sweeps if n_sweeps is None else int(n_sweeps)
        dt, sc, gt = self._classes.step_rows(params, scores, categories, batch_index, annotations, n_sweeps, n_cat)
        stray = (~dt.inside).sum() + (~gt.inside).sum()  # the AV2 rule: only the sweep decides (the class docstring)
        gt_valid = None if num_interior_pts is None else (num_interior_pts.to(dev).reshape(-1) > 0).to(torch.uint8).contiguous()
        if self._n_gt is None:
            self._n_gt = torch.zeros(n_cat + 1, dtype=torch.int64, device=dev)
            self._stray = torch.zeros((), dtype=torch.int64, device=dev)
        dt_roi = None
        if roi is not None:
            from ..converters.av2.roi import roi_boxes

            if self.atlas.device != dev:
                self.atlas = self.atlas.to(dev)
            layer_index, city_SE3_ego = roi
            # (rows outside the step's sweeps are counted above already: these launches count into a spare)
            spare = torch.zeros((), dtype=torch.int64, device=dev)
            dt_roi = roi_boxes(dt.rows, dt.sweep, layer_index, city_SE3_ego, self.atlas, stray=spare)
            gt_roi = roi_boxes(gt.rows, gt.sweep, layer_index, city_SE3_ego, self.atlas, stray=spare)
            gt_valid = gt_roi if gt_valid is None else gt_valid & gt_roi
        out = match(dt.rows, sc, dt.segment, gt.rows, gt_valid, gt.segment, n_sweeps * n_cat, self.cfg, dt_roi=dt_roi)
        self._append({"score": sc, "category": dt.group, "evaluated": out["evaluated"], "tp": out["tp"], "err": out["err"]})
        # (ground truth of a class that is not evaluated is never flagged: its slot is the spare one at the end)
        self._n_gt.index_add_(0, torch.where(gt.group >= 0, gt.group, n_cat), out["gt_evaluated"].to(torch.int64))
        self._stray += stray

    def _gathered(self) -> Tuple[Dict[str, Tensor], Tensor, Tensor]:
        """The accumulators, concatenated over the ranks when ``torch.distributed`` is initialised (rank order; sizes first,
        rows padded to the longest)."""
        import torch.distributed as dist

        rows = {k: v[:self._n] for k, v in self._buf.items()}
        if not (dist.is_available() and dist.is_initialized()):
            return rows, self._n_gt[:-1], self._stray
        world, dev = dist.get_world_size(), self._n_gt.device
        sizes = [torch.zeros((), dtype=torch.int64, device=dev) for _ in range(world)]
        dist.all_gather(sizes, torch.tensor(self._n, dtype=torch.int64, device=dev))
        sizes = [int(s) for s in sizes]
        longest = max(sizes)
        gathered = {}
        for name, t in rows.items():
            padded = torch.zeros((longest,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            padded[:self._n].copy_(t)
            parts = [torch.empty_like(padded) for _ in range(world)]
            dist.all_gather(parts, padded)
            gathered[name] = torch.cat([p[:s] for p, s in zip(parts, sizes)])
        counts = torch.cat([self._n_gt[:-1], self._stray.reshape(1)])
        dist.all_reduce(counts)
        return gathered, counts[:-1], counts[-1]

    def compute(self):
        """The metric table of everything seen since ``reset`` (every rank's, under ``torch.distributed``): an Arrow table with the
        columns ``category, AP, ATE, ASE, AOE, CDS, n_dts, n_gts``, one row per ``cfg.categories`` and ``AVERAGE_METRICS`` last."""
        if self._n_gt is None:
            raise L.RvError("DetectionEvaluator.compute() before any update()")
        rows, n_gt, stray = self._gathered()
        if int(stray) != 0:
            raise L.RvError(stray_rows_message(int(stray), self.max_sweeps))
        n_gt = n_gt.contiguous()
        table, _, n_dts = summarize(rows["score"], rows["category"], rows["evaluated"], rows["tp"], rows["err"], n_gt, self.cfg)
        return _metrics_table(self.cfg, table, n_dts, n_gt.cpu())


def evaluate(dts, gts, cfg: DetectionCfg, device: Any = "cuda", atlas=None, poses: Optional[Mapping[Tuple[str, int], Any]] = None):
    """The offline form, mirroring ``_, _, metrics = evaluate(dts, gts, cfg)`` (``detector.py:472``): ``dts`` is what
    ``write_detections`` wrote, concatenated (``DETECTION_COLUMNS``, ``score``, ``log_id``, ``timestamp_ns``, ``category``),
    ``gts`` has the ``annotations.feather`` schema (``DETECTION_COLUMNS``, ``category``, ``num_interior_pts``, ``log_id``,
    ``timestamp_ns``); sweeps are the (``log_id``, ``timestamp_ns``) groups.  Returns ``(dts, gts, metrics)``: ``dts`` with
    ``is_evaluated``, one ``tp_<threshold>`` flag column per affinity threshold and ``ATE`` / ``ASE`` / ``AOE`` (NaN where the row is
    not a true positive at ``tp_threshold_m``) appended, ``gts`` with ``is_evaluated``, ``metrics`` as ``DetectionEvaluator.compute``.

    With ``cfg.eval_only_roi_instances``: ``atlas`` (``converters.av2.roi.RoiAtlas``; a sweep's layer is found by its ``log_id``) and
    ``poses``, mapping ``(log_id, timestamp_ns)`` to that sweep's ``city_SE3_ego`` as a (3, 4) array; a sweep without a pose raises and
    names it.  The returned ``dts`` / ``gts`` then also carry ``is_within_roi``."""
    import numpy as np
    import pyarrow as pa

    _check_cfg(cfg)
    _check_roi(cfg, "atlas / poses", atlas, poses)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.RvError(f"evaluate() on {dev}: the evaluation kernels only run on an MI355X (no CPU fallback)")
    n_cat = len(cfg.categories)
    sweeps: Dict[Tuple[str, int], int] = {}
    cat_index = {c: i for i, c in enumerate(cfg.categories)}

    def rows_of(frame):
        cat = [cat_index.get(str(c), -1) for c in _column(frame, "category")]
        return (torch.from_numpy(frame_rows(frame)).to(dev), torch.from_numpy(sweep_index(frame, sweeps)).to(dev),
                torch.tensor(cat, dtype=torch.int64, device=dev))

    dt_box, dt_sweep, dt_cat = rows_of(dts)
    gt_box, gt_sweep, gt_cat = rows_of(gts)
    n_seg = max(len(sweeps), 1) * n_cat
    score = torch.tensor(np.asarray(_column(dts, "score"), dtype=np.float32), device=dev)
    gt_valid = (torch.tensor(np.asarray(_column(gts, "num_interior_pts"), dtype=np.int64), device=dev) > 0).to(torch.uint8)
    dt_roi = gt_roi = None
    if cfg.eval_only_roi_instances and sweeps:
        from ..converters.av2.roi import roi_boxes

        missing = [key for key in sweeps if key not in poses]
        if missing:
            raise L.RvError(f"no city_SE3_ego for sweep (log_id, timestamp_ns) = {missing[0]} ({len(missing)} of {len(sweeps)} sweeps lack a pose)")
        layer_index = torch.tensor([atlas.layer_of(log_id) for log_id, _ in sweeps], dtype=torch.int32)
        city_SE3_ego = torch.from_numpy(np.stack([np.asarray(poses[key], dtype=np.float64).reshape(-1)[:12].reshape(3, 4) for key in sweeps]))
        atlas = atlas.to(dev)
        dt_roi = roi_boxes(dt_box, dt_sweep, layer_index, city_SE3_ego, atlas)
        gt_roi = roi_boxes(gt_box, gt_sweep, layer_index, city_SE3_ego, atlas)
        gt_valid = gt_valid & gt_roi
    elif cfg.eval_only_roi_instances:  # (no rows at all)
        dt_roi, gt_roi = torch.zeros(0, dtype=torch.uint8, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev)
    out = match(dt_box, score, torch.where(dt_cat >= 0, dt_sweep * n_cat + dt_cat, n_seg), gt_box, gt_valid,
                torch.where(gt_cat >= 0, gt_sweep * n_cat + gt_cat, n_seg), n_seg, cfg, dt_roi=dt_roi)
    n_gt = torch.zeros(n_cat + 1, dtype=torch.int64, device=dev)
    n_gt.index_add_(0, torch.where(gt_cat >= 0, gt_cat, n_cat), out["gt_evaluated"].to(torch.int64))
    n_gt = n_gt[:-1].contiguous()
    table, _, n_dts = summarize(score, dt_cat, out["evaluated"], out["tp"], out["err"], n_gt, cfg)
    tp, err = out["tp"].cpu().numpy(), out["err"].cpu().numpy()
    dts_out = dts.append_column("is_evaluated", pa.array(out["evaluated"].cpu().numpy().astype(bool)))
    for j, t in enumerate(cfg.affinity_thresholds_m):
        dts_out = dts_out.append_column(f"tp_{t}", pa.array(np.ascontiguousarray(tp[:, j]).astype(bool)))
    for j, name in enumerate(("ATE", "ASE", "AOE")):
        dts_out = dts_out.append_column(name, pa.array(np.ascontiguousarray(err[:, j]), type=pa.float32(), from_pandas=False))
    gts_out = gts.append_column("is_evaluated", pa.array(out["gt_evaluated"].cpu().numpy().astype(bool)))
    if dt_roi is not None:
        dts_out = dts_out.append_column("is_within_roi", pa.array(dt_roi.cpu().numpy().astype(bool)))
        gts_out = gts_out.append_column("is_within_roi", pa.array(gt_roi.cpu().numpy().astype(bool)))
    return dts_out, gts_out, _metrics_table(cfg, table, n_dts, n_gt.cpu())
