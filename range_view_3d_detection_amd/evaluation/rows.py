"""The front end both evaluators share, in plain torch on whatever device the rows are on: what ``RangeDecoder.decode`` returned and the
loader's (M,13) annotation rows become rows labelled with a (sweep, group) segment (``ClassMap.step_rows``), the rows are ordered by
(segment, score descending) with segment offsets (``order_rows``), and the kernels walk ``order[off[seg] .. off[seg + 1])`` with clamped
offsets and guarded row indices (``csrc/segments.h``).  Every output has a fixed size: nothing here reads anything back.

The AV2 metric groups by row of ``cfg.categories`` (:mod:`.detection`), the Waymo one by object type - 1 (:mod:`.waymo`).
"""

from __future__ import annotations

from typing import Dict, Mapping, NamedTuple, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from ..math.ops.coding import DETECTION_COLUMNS, _column


def sort_key(segment: Tensor, scores: Tensor) -> Tensor:
    """int64 key that orders rows by (segment ascending, score descending) under ONE stable ascending sort: the segment in the
    high word, the complement of the score's order-preserving bit pattern in the low word (-0.0 counts as +0.0)."""
    bits = (scores.float() + 0.0).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    ascending = torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)
    return (segment << 32) | (0xFFFFFFFF - ascending)


def segment_offsets(sorted_keys: Tensor, n: int, shift: int) -> Tensor:
    """(n + 1) offsets of the segments 0 .. n - 1 in a sorted key array (a fixed-size output: nothing is read back)."""
    bounds = torch.arange(n + 1, dtype=torch.int64, device=sorted_keys.device) << shift
    return torch.searchsorted(sorted_keys, bounds)


def order_rows(dt_segment: Tensor, scores: Tensor, gt_segment: Tensor, n_segments: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(dt_order, dt_off, gt_order, gt_off)``: the detections by (segment ascending, score descending, ties in input order), the
    ground truth by segment (stable), and the (n_segments + 1) offsets of the segments in either list.  Rows of a segment outside
    ``[0, n_segments)`` lie before ``off[0]`` or from ``off[n_segments]`` on."""
    sorted_keys, dt_order = torch.sort(sort_key(dt_segment, scores), stable=True)
    gt_sorted, gt_order = torch.sort(gt_segment, stable=True)
    return dt_order, segment_offsets(sorted_keys, n_segments, 32), gt_order, segment_offsets(gt_sorted, n_segments, 0)


def task_bases(idx_to_category, tasks: Optional[Mapping[int, Sequence[str]]]) -> Tuple[Tuple[str, ...], Dict[int, int]]:
    """Category names in class-index order and, per task id, the class index of its offset 0: ``DetectionHead`` numbers the
    classes task after task (``RangeDecoder.decode``'s ``category_offset``)."""
    if isinstance(idx_to_category, (list, tuple)):
        names = tuple(str(c) for c in idx_to_category)
        task_ids = offsets = None
    else:
        names = tuple(str(c) for c in _column(idx_to_category, "category"))
        try:
            task_ids, offsets = _column(idx_to_category, "task_id"), _column(idx_to_category, "offset")
        except (KeyError, AttributeError):
            task_ids = offsets = None
    bases: Dict[int, int] = {}
    if tasks is not None:
        base = 0
        for task_id, group in tasks.items():
            bases[int(task_id)] = base
            base += len(group)
        if base != len(names):
            raise L.RvError(f"the task table holds {base} categories, idx_to_category {len(names)}")
    elif task_ids is not None:
        for i, (t, o) in enumerate(zip(task_ids, offsets)):
            if int(o) == 0:
                bases[int(t)] = i
    else:
        bases[0] = 0  # one task
    return names, bases


class Side(NamedTuple):
    """One side (detections or ground truth) of a step, every field in input row order."""

    rows: Tensor     # (n, 10) f32, DETECTION_COLUMNS order
    sweep: Tensor    # (n,) i64 batch_index as given
    group: Tensor    # (n,) i64 group of the row's class, -1: unknown class or a class that is not evaluated
    segment: Tensor  # (n,) i64 sweep * n_groups + group, or n_sweeps * n_groups = no segment
    inside: Tensor   # (n,) bool: 0 <= sweep < n_sweeps
    known: Tensor    # (n,) bool: the class index (for ground truth: task id, its base and the sum) names a class of the table


class ClassMap:
    """Class index -> group (-1: not evaluated) and task id -> class index of offset 0, as lookup tensors per device.  Configuration,
    not state: an evaluator keeps it over ``reset()``, so only the first ``step_rows`` on a device copies anything to it."""

    def __init__(self, class_to_group: Sequence[int], bases: Mapping[int, int]) -> None:
        self._group = [int(g) for g in class_to_group]
        self._base = [-1] * (max(bases) + 1)
        for t, b in bases.items():
            self._base[t] = b
        self._lut: Optional[Tuple[Tensor, Tensor]] = None

    def step_rows(self, params: Tensor, scores: Tensor, categories: Tensor, batch_index: Tensor, annotations: Tensor, n_sweeps: int,
                  n_groups: int) -> Tuple[Side, Tensor, Side]:
        """One validation step -> ``(detections, scores (N,) f32, ground truth)``.  ``params`` (N,10), ``scores``, ``categories`` and
        ``batch_index`` (N,) are floats or integers, ``annotations`` the (M,13) rows of ``prototype.loader.COLS`` (box, ``task_id``,
        ``offset``, ``batch_index``), moved to ``params``' device.  A row has a segment where it is inside and its group is >= 0."""
        dev = params.device
        if self._lut is None or self._lut[0].device != dev:
            self._lut = (torch.tensor(self._group, dtype=torch.int64, device=dev), torch.tensor(self._base, dtype=torch.int64, device=dev))
        group_of, task_base = self._lut
        n_cls, none = group_of.shape[0], n_sweeps * n_groups

        def side(rows: Tensor, sweep: Tensor, cls: Tensor, known: Tensor) -> Side:
            known = known & (cls >= 0) & (cls < n_cls)
            group = torch.where(known, group_of[cls.clamp(0, n_cls - 1)], -1)
            inside = (sweep >= 0) & (sweep < n_sweeps)
            return Side(rows, sweep, group, torch.where(inside & (group >= 0), sweep * n_groups + group, none), inside, known)

        cls = categories.detach().reshape(-1).to(torch.int64)
        dts = side(params.detach().float().reshape(-1, 10).contiguous(), batch_index.detach().reshape(-1).to(torch.int64), cls,
                   torch.ones_like(cls, dtype=torch.bool))
        ann = annotations.detach().to(dev).reshape(-1, 13)  # (the loader's rows are host tensors: a copy, no read-back)
        task = ann[:, 10].to(torch.int64)
        base = task_base[task.clamp(0, task_base.shape[0] - 1)]
        gts = side(ann[:, :10].float().contiguous(), ann[:, 12].to(torch.int64), base + ann[:, 11].to(torch.int64),
                   (task >= 0) & (task < task_base.shape[0]) & (base >= 0))
        return dts, scores.detach().float().reshape(-1).contiguous(), gts


def stray_rows_message(stray: int, max_sweeps: int) -> str:
    return (f"{stray} rows had a batch_index outside [0, n_sweeps): pass the step's batch size to update() "
            f"(or a larger max_sweeps, now {max_sweeps})")


def frame_rows(frame):
    """(n, 10) fp32 NumPy rows in ``DETECTION_COLUMNS`` order of an Arrow table (or a mapping of columns); (0, 10) without rows."""
    import numpy as np

    return np.stack([np.asarray(_column(frame, c), dtype=np.float32) for c in DETECTION_COLUMNS], 1)


def sweep_index(frame, sweeps: Dict[Tuple[str, int], int], add: bool = True, keep=None):
    """int64 NumPy index of every row's (``log_id``, ``timestamp_ns``) sweep in ``sweeps``.  With ``add`` a sweep not seen before gets
    the next number (order of first appearance); without, its rows get -1 and ``sweeps`` stays as it is.  A row whose ``keep`` is
    false gets -1 and numbers nothing."""
    import numpy as np

    keys = [(str(l), int(t)) for l, t in zip(_column(frame, "log_id"), _column(frame, "timestamp_ns"))]
    keep = [True] * len(keys) if keep is None else keep
    return np.asarray([-1 if not k else sweeps.setdefault(key, len(sweeps)) if add else sweeps.get(key, -1) for key, k in zip(keys, keep)],
                      dtype=np.int64)
