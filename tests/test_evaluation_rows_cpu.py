"""The evaluators' shared front end (``evaluation/rows.py``) on the CPU: the ordering against ``numpy.lexsort``, ``ClassMap.step_rows``
against a plain loop over the rows with both stray rules, and the offline forms' ``frame_rows`` / ``sweep_index``."""

from __future__ import annotations

import numpy as np
import pytest
import torch

N_SEG = 6


def _order_case():
    g = np.random.default_rng(11)
    n, m = 200, 90
    scores = np.round(g.uniform(-0.3, 1.0, n), 2).astype(np.float32)  # a 0.01 grid: ties, negative scores
    scores[:12] = [0.0, -0.0, 0.0, -0.0] * 3
    dt_seg = g.choice([0, 1, 2, 4, 5, N_SEG], n)  # segment 3 is empty, N_SEG = no segment
    dt_seg[:12] = 2  # the signed zeros meet in one segment
    gt_seg = g.choice([0, 1, 2, 4, 5, N_SEG], m)
    return scores, dt_seg.astype(np.int64), gt_seg.astype(np.int64)


def test_order_rows_against_lexsort():
    from range_view_3d_detection_amd.evaluation.rows import order_rows

    scores, dt_seg, gt_seg = _order_case()
    assert np.signbit(scores[1]) and not np.signbit(scores[0]) and (scores < 0).sum() > 10 and len(np.unique(scores)) < 140
    dt_order, dt_off, gt_order, gt_off = [t.numpy() for t in order_rows(torch.from_numpy(dt_seg), torch.from_numpy(scores),
                                                                        torch.from_numpy(gt_seg), N_SEG)]
    # segment ascending, score descending, input order on ties (-0.0 == 0.0 under the comparison lexsort makes)
    assert np.array_equal(dt_order, np.lexsort((np.arange(len(scores)), -scores, dt_seg)))
    zeros = dt_order[np.isin(dt_order, np.arange(12))]
    assert np.array_equal(zeros, np.arange(12))  # the signed zeros tie: input order
    assert np.array_equal(gt_order, np.argsort(gt_seg, kind="stable"))
    for off, seg in ((dt_off, dt_seg), (gt_off, gt_seg)):
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(seg, minlength=N_SEG + 1)[:N_SEG])]))
        assert off[3] == off[4] and off[N_SEG] < len(seg)  # the empty segment; rows of no segment lie behind the last offset


def test_order_rows_without_rows():
    from range_view_3d_detection_amd.evaluation.rows import order_rows

    scores, dt_seg, gt_seg = _order_case()
    none_i, none_f = torch.zeros(0, dtype=torch.int64), torch.zeros(0)
    dt_order, dt_off, gt_order, gt_off = order_rows(none_i, none_f, torch.from_numpy(gt_seg), N_SEG)  # n = 0
    assert dt_order.numel() == 0 and dt_off.tolist() == [0] * (N_SEG + 1) and gt_off[N_SEG] > 0
    dt_order, dt_off, gt_order, gt_off = order_rows(torch.from_numpy(dt_seg), torch.from_numpy(scores), none_i, N_SEG)  # m = 0
    assert gt_order.numel() == 0 and gt_off.tolist() == [0] * (N_SEG + 1) and dt_off[N_SEG] > 0


# (class index, sweep) of the detections and (task id, offset, sweep) of the annotations; 3 sweeps, 3 classes A B C
N_SWEEPS, N_GROUPS = 3, 2
GROUPS = [0, -1, 1]  # B is a class that is not evaluated (the AV2 case)
DT_ROWS = [(0, 0), (1, 1), (2, 2), (-1, 0), (3, 1), (0, -1), (2, 3), (5, -1), (2, 0)]
GT_ROWS = [(0, 0, 0), (0, 1, 1), (1, 0, 2), (2, 0, 0), (-1, 0, 1), (0, 5, 1), (0, -1, 1), (0, 0, -1), (0, 0, 3), (3, 0, 0), (1, 0, -1)]
# configuration -> (idx_to_category, tasks, ground-truth rows that are stray under the Waymo rule)
CONFIGS = {
    "one-task-list": (["A", "B", "C"], None, 9),  # tasks 1, 2, 3 are past the table
    "two-task-table": (["A", "B", "C"], {0: ["A", "B"], 1: ["C"]}, 8),  # task 1 starts at C
    "task-frame": ({"category": ["A", "B", "C"], "task_id": [0, 0, 2], "offset": [0, 1, 0]}, None, 8),  # task 1 has no class: base -1
}


def _loop(bases):
    """The declaration, row by row: (group, segment, inside, known) per side."""
    base_of = [-1] * (max(bases) + 1)
    for t, b in bases.items():
        base_of[t] = b
    none = N_SWEEPS * N_GROUPS

    def row(cls, sweep, known):
        known = known and 0 <= cls < len(GROUPS)
        group = GROUPS[cls] if known else -1
        inside = 0 <= sweep < N_SWEEPS
        return group, sweep * N_GROUPS + group if inside and group >= 0 else none, inside, known

    dts = [row(c, s, True) for c, s in DT_ROWS]
    gts = []
    for task, offset, sweep in GT_ROWS:
        known = 0 <= task < len(base_of) and base_of[task] >= 0
        gts.append(row(base_of[task] + offset if known else -1, sweep, known))
    return dts, gts


@pytest.mark.parametrize("name", list(CONFIGS))
def test_step_rows_against_a_loop_over_the_rows(name):
    from range_view_3d_detection_amd.evaluation.rows import ClassMap, task_bases

    idx_to_category, tasks, want_waymo_gt = CONFIGS[name]
    names, bases = task_bases(idx_to_category, tasks)
    assert names == ("A", "B", "C")
    g = torch.Generator().manual_seed(3)
    params, scores = torch.randn(len(DT_ROWS), 10, generator=g, dtype=torch.float64), torch.rand(len(DT_ROWS), generator=g, dtype=torch.float64)
    categories = torch.tensor([float(c) for c, _ in DT_ROWS])  # floats, as ``RangeDecoder.decode`` returns them
    batch_index = torch.tensor([float(s) for _, s in DT_ROWS])
    ann = torch.randn(len(GT_ROWS), 13, generator=g, dtype=torch.float64)
    ann[:, 10:] = torch.tensor(GT_ROWS, dtype=torch.float64)
    classes = ClassMap(GROUPS, bases)
    classes.step_rows(params[:0], scores[:0], categories[:0], batch_index[:0], ann[:0], N_SWEEPS, N_GROUPS)
    lut = classes._lut
    dt, sc, gt = classes.step_rows(params, scores, categories, batch_index, ann, N_SWEEPS, N_GROUPS)
    assert classes._lut is lut  # the lookup tensors are built once per device
    assert dt.rows.dtype == sc.dtype == gt.rows.dtype == torch.float32
    assert torch.equal(dt.rows, params.float()) and torch.equal(sc, scores.float()) and torch.equal(gt.rows, ann[:, :10].float())
    assert dt.sweep.tolist() == [s for _, s in DT_ROWS] and gt.sweep.tolist() == [s for _, _, s in GT_ROWS]
    for side, want in zip((dt, gt), _loop(bases)):
        assert side.group.tolist() == [w[0] for w in want]
        assert side.segment.tolist() == [w[1] for w in want]
        assert side.inside.tolist() == [w[2] for w in want] and side.known.tolist() == [w[3] for w in want]
        assert side.segment.dtype == side.group.dtype == torch.int64
    assert dt.segment.tolist() == [0, 6, 5, 6, 6, 6, 6, 6, 1]  # (B has no segment)
    # AV2: only the sweep decides; Waymo: the sweep and the class
    assert (int((~dt.inside).sum()), int((~gt.inside).sum())) == (3, 3)
    assert (int((~(dt.inside & dt.known)).sum()), int((~(gt.inside & gt.known)).sum())) == (5, want_waymo_gt)


def _frame(logs, stamps, first):
    import pyarrow as pa

    from range_view_3d_detection_amd.math.ops.coding import DETECTION_COLUMNS

    n = len(logs)
    cols = {c: pa.array(np.arange(n, dtype=np.float64) + first + 0.25 * j) for j, c in enumerate(DETECTION_COLUMNS)}
    return pa.table({**cols, "log_id": pa.array(logs, type=pa.string()), "timestamp_ns": pa.array(stamps, type=pa.int64())})


def test_frame_rows_and_sweep_index():
    from range_view_3d_detection_amd.evaluation.rows import frame_rows, sweep_index

    empty, three = _frame([], [], 0), _frame(["b", "a", "b"], [7, 7, 7], 10)
    rows = frame_rows(empty)
    assert rows.shape == (0, 10) and rows.dtype == np.float32
    rows = frame_rows(three)
    assert rows.dtype == np.float32 and np.array_equal(rows, (np.arange(3)[:, None] + 10 + 0.25 * np.arange(10)[None]).astype(np.float32))
    sweeps = {}
    assert sweep_index(empty, sweeps).shape == (0,) and sweeps == {}
    index = sweep_index(three, sweeps)
    assert index.dtype == np.int64 and index.tolist() == [0, 1, 0] and sweeps == {("b", 7): 0, ("a", 7): 1}  # order of first appearance
    other = _frame(["a", "c", "b"], [7, 7, 8], 0)
    assert sweep_index(other, sweeps, add=False).tolist() == [1, -1, -1] and len(sweeps) == 2
    assert sweep_index(other, sweeps, keep=[False, True, True]).tolist() == [-1, 2, 3] and sweeps[("c", 7)] == 2 and sweeps[("b", 8)] == 3
