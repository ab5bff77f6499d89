"""NumPy restatement of the declared detection-evaluation semantics (include/rv3d.h): plain loops over sweeps and
categories, float64, ``np.interp``, ``np.maximum.accumulate``.  Written from the declaration, not from the kernels; the tests
compare ``rv_eval_match`` / ``rv_eval_summarize`` against it and it against the hand-computed cases of
``tests/golden/eval_cases.json``.

Rows are (n, 10) float32 ``[tx_m, ty_m, tz_m, length_m, width_m, height_m, qw, qx, qy, qz]``.  ``cfg`` is anything with the
attributes of ``DetectionCfg``.
"""

from __future__ import annotations

import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rows_from_yaw(rows) -> np.ndarray:
    """(n, 7) [x, y, z, l, w, h, yaw] -> (n, 10) float32 rows with the quaternion [cos(yaw/2), 0, 0, sin(yaw/2)]."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, 7)
    out = np.zeros((r.shape[0], 10), dtype=np.float32)
    out[:, :6] = r[:, :6]
    out[:, 6] = np.cos(r[:, 6] / 2)
    out[:, 9] = np.sin(r[:, 6] / 2)
    return out


def _norm2(xyz: np.ndarray) -> np.ndarray:
    p = xyz.astype(np.float64)
    return (p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2]


def _yaw(rows: np.ndarray) -> np.ndarray:
    return 2.0 * np.arctan2(rows[..., 9].astype(np.float64), rows[..., 6].astype(np.float64))


def match_ref(dts, scores, dt_sweep, dt_cat, gts, gt_valid, gt_sweep, gt_cat, n_sweeps, n_cat, cfg):
    """Steps 1-5 of the declaration.  Returns ``evaluated`` (N,) u8, ``tp`` (N, T) u8, ``err`` (N, 3) f64 (NaN where not a
    true positive at ``tp_threshold_m``), ``matched_gt`` (N,) i32, ``gt_evaluated`` (M,) u8."""
    dts, gts = np.asarray(dts, np.float32).reshape(-1, 10), np.asarray(gts, np.float32).reshape(-1, 10)
    scores = np.asarray(scores, np.float32)
    dt_sweep, dt_cat, gt_sweep, gt_cat = (np.asarray(v) for v in (dt_sweep, dt_cat, gt_sweep, gt_cat))
    n, m, thr = len(dts), len(gts), [float(t) for t in cfg.affinity_thresholds_m]
    r2 = float(cfg.max_range_m) * float(cfg.max_range_m)
    evaluated, tp = np.zeros(n, np.uint8), np.zeros((n, len(thr)), np.uint8)
    err, matched = np.full((n, 3), np.nan), np.full(n, -1, np.int32)
    gt_ok = (_norm2(gts[:, :3]) <= r2) & (np.ones(m, bool) if gt_valid is None else np.asarray(gt_valid) != 0)
    gt_evaluated = np.zeros(m, np.uint8)
    for s in range(n_sweeps):
        for c in range(n_cat):
            g_rows = np.nonzero((gt_sweep == s) & (gt_cat == c) & gt_ok)[0].tolist()
            gt_evaluated[g_rows] = 1
            d_rows = np.nonzero((dt_sweep == s) & (dt_cat == c))[0]
            if len(d_rows) == 0:
                continue
            d_rows = d_rows[_norm2(dts[d_rows, :3]) <= r2]
            d_rows = d_rows[np.argsort(-scores[d_rows], kind="stable")][: cfg.max_num_dts_per_category]
            evaluated[d_rows] = 1
            taken = set()
            for i in d_rows:
                if not g_rows:
                    break
                diff = dts[i, :3].astype(np.float64) - gts[g_rows, :3].astype(np.float64)
                d2 = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
                k = int(np.argmin(d2))  # first minimum: the lowest ground-truth index
                j = g_rows[k]
                if j in taken:
                    continue  # its nearest box is gone: unmatched, no second choice
                taken.add(j)
                matched[i] = j
                for t, v in enumerate(thr):
                    tp[i, t] = d2[k] <= v * v
                if d2[k] <= float(cfg.tp_threshold_m) ** 2:
                    a, b = dts[i, 3:6].astype(np.float64), gts[j, 3:6].astype(np.float64)
                    dyaw = abs(float(_yaw(dts[i]) - _yaw(gts[j]))) % (2 * math.pi)
                    err[i] = (math.sqrt(d2[k]), 1.0 - np.minimum(a, b).prod() / np.maximum(a, b).prod(), min(dyaw, 2 * math.pi - dyaw))
    return {"evaluated": evaluated, "tp": tp, "err": err, "matched_gt": matched, "gt_evaluated": gt_evaluated}


def summarize_ref(scores, cats, evaluated, tp, err, n_gt, n_cat, cfg):
    """The per-category reduction: (n_cat + 1, 5) table [AP, ATE, ASE, AOE, CDS] (last row: column means) and AP per threshold."""
    scores, cats, evaluated = np.asarray(scores, np.float32), np.asarray(cats), np.asarray(evaluated)
    tp, err = np.asarray(tp), np.asarray(err, np.float64)
    n_thr = tp.shape[1]
    table, ap_t = np.zeros((n_cat + 1, 5)), np.zeros((n_cat, n_thr))
    tp_thr = float(cfg.tp_threshold_m)
    for c in range(n_cat):
        rows = np.nonzero((cats == c) & (evaluated != 0))[0]
        rows = rows[np.argsort(-scores[rows], kind="stable")]
        if len(rows) and n_gt[c] > 0:
            for t in range(n_thr):
                flag = tp[rows, t] != 0
                tps, fps = np.cumsum(flag), np.cumsum(~flag)
                recall, precision = tps / float(n_gt[c]), tps / (tps + fps)
                precision = np.maximum.accumulate(precision[::-1])[::-1]
                samples = np.interp(np.linspace(0, 1, cfg.num_recall_samples), recall, precision, left=precision[0], right=0)
                ap_t[c, t] = samples.mean()
        ap = ap_t[c].mean()
        e = err[rows]
        e = e[~np.isnan(e[:, 0])] if len(rows) else e
        ate, ase, aoe = e.mean(0) if len(e) else (tp_thr, 1.0, math.pi)
        cds = ap * np.mean([1 - min(ate / tp_thr, 1), 1 - min(ase, 1), 1 - min(aoe / math.pi, 1)])
        table[c] = (ap, ate, ase, aoe, cds)
    table[n_cat] = table[:n_cat].mean(0)
    return table, ap_t


def evaluate_ref(dts, scores, dt_sweep, dt_cat, gts, gt_valid, gt_sweep, gt_cat, n_sweeps, n_cat, cfg):
    out = match_ref(dts, scores, dt_sweep, dt_cat, gts, gt_valid, gt_sweep, gt_cat, n_sweeps, n_cat, cfg)
    n_gt = np.array([int(np.sum((np.asarray(gt_cat) == c) & (out["gt_evaluated"] != 0))) for c in range(n_cat)])
    table, ap_t = summarize_ref(scores, dt_cat, out["evaluated"], out["tp"], out["err"], n_gt, n_cat, cfg)
    return out, n_gt, table, ap_t


def load_cases():
    """The hand-computed cases of ``tests/golden/eval_cases.json`` as arrays: per case a dict with ``dts`` / ``gts`` (n, 10) f32,
    ``scores``, ``dt_sweep``, ``dt_cat``, ``gt_valid``, ``gt_sweep``, ``gt_cat``, ``n_sweeps``, ``n_cat`` and ``expect``
    (``evaluated``, ``tp``, ``matched_gt``, ``err`` with NaN rows, ``gt_evaluated``, ``table``)."""
    cases = []
    for raw in json.load(open(os.path.join(GOLDEN, "eval_cases.json")))["cases"]:
        d_rows = [list(r) for r in raw.get("dts", [])]
        gen = raw.get("dts_generated")
        if gen:  # `count` copies of `row`, score of row i = i / score_denominator, single rows replaced by `override`
            for i in range(gen["count"]):
                d_rows.append(list(gen["override"].get(str(i), gen["row"])) + [i / gen["score_denominator"], gen["sweep"], gen["category"]])
        d, g = np.asarray(d_rows, np.float64).reshape(-1, 10), np.asarray(raw["gts"], np.float64).reshape(-1, 10)
        exp, n_thr = dict(raw["expect"]), 4
        if "evaluated_from" in exp:  # rows below it are not evaluated, `matched_row` is the one match, no true positives
            n = len(d)
            exp["evaluated"] = [int(i >= exp["evaluated_from"]) for i in range(n)]
            exp["tp"] = [[0] * n_thr for _ in range(n)]
            exp["matched_gt"] = [0 if i == exp["matched_row"] else -1 for i in range(n)]
            exp["err"] = [None] * n
        exp["err"] = np.array([[np.nan] * 3 if e is None else e for e in exp["err"]], np.float64).reshape(-1, 3)
        cases.append({"name": raw["name"], "n_sweeps": raw["n_sweeps"], "n_cat": raw["n_categories"],
                      "dts": rows_from_yaw(d[:, :7]), "scores": d[:, 7].astype(np.float32), "dt_sweep": d[:, 8].astype(np.int64),
                      "dt_cat": d[:, 9].astype(np.int64), "gts": rows_from_yaw(g[:, :7]), "gt_valid": (g[:, 7] > 0).astype(np.uint8),
                      "gt_sweep": g[:, 8].astype(np.int64), "gt_cat": g[:, 9].astype(np.int64), "expect": exp})
    return cases
