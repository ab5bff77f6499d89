"""NumPy restatement of the Waymo detection metric as ``include/rv3d.h`` declares it (``rv_waymo_iou`` / ``rv_waymo_match`` /
``rv_waymo_summarize``), written from the header: float64 polygon clipping for the IoU, the sequential insertion procedure on
integers, the counts, AP / APH.  Slow and plain on purpose; nothing here is compacted or parallel."""

from __future__ import annotations

import json
import math
import os

import numpy as np

TYPES = {"VEHICLE": 1, "PEDESTRIAN": 2, "SIGN": 3, "CYCLIST": 4}
THRESHOLDS = np.asarray([0.0, 0.7, 0.5, 0.5, 0.5], np.float32)
CUTOFFS = np.asarray([np.float32(k * 0.01) for k in range(100)] + [np.float32(1.0)], np.float32)
N_CUT, N_BROWS, N_RROWS = 101, 16, 32
START, NONE = -2, -1
QUANTUM = 2.0 ** 40


# ----------------------------------------------------------------------------------------------------------------------
# boxes
# ----------------------------------------------------------------------------------------------------------------------
def rows_from_yaw(boxes7) -> np.ndarray:
    """(n,7) [x,y,z,l,w,h,yaw] -> (n,10) fp32 rows with the quaternion of a rotation about z."""
    b = np.asarray(boxes7, np.float64).reshape(-1, 7)
    zero = np.zeros(len(b))
    return np.concatenate([b[:, :6], np.stack([np.cos(b[:, 6] / 2), zero, zero, np.sin(b[:, 6] / 2)], 1)], 1).astype(np.float32)


def boxes_from_rows(rows10) -> np.ndarray:
    r = np.asarray(rows10, np.float32).astype(np.float64).reshape(-1, 10)
    qw, qx, qy, qz = r[:, 6], r[:, 7], r[:, 8], r[:, 9]
    yaw = np.arctan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz))
    return np.concatenate([r[:, :6], yaw[:, None]], 1).astype(np.float32)


def level_of(num_interior_pts: int, difficulty_level: int = 0) -> int:
    if num_interior_pts <= 0:
        return 0
    return int(difficulty_level) if difficulty_level != 0 else (2 if num_interior_pts <= 5 else 1)


def range_shard(box) -> int:
    x, y, z = (float(np.float32(v)) for v in box[:3])
    r2 = (x * x + y * y) + z * z
    return 1 if r2 < 900.0 else 2 if r2 < 2500.0 else 3 if r2 >= 2500.0 else 0


def cutoff_index(score) -> int:
    hit = np.flatnonzero(np.float32(score) >= CUTOFFS)
    return int(hit[-1]) if len(hit) else -1


# ----------------------------------------------------------------------------------------------------------------------
# IoU: float64 clipping
# ----------------------------------------------------------------------------------------------------------------------
def _corners(box):
    x, y, l, w, yaw = float(box[0]), float(box[1]), float(box[3]), float(box[4]), float(box[6])
    c, s = math.cos(yaw), math.sin(yaw)
    return [(x + dx * c - dy * s, y + dx * s + dy * c) for dx, dy in ((l / 2, w / 2), (-l / 2, w / 2), (-l / 2, -w / 2), (l / 2, -w / 2))]


def _clip_area(pa, pb) -> float:
    poly = list(pa)
    for e in range(4):
        (ax, ay), (bx, by) = pb[e], pb[(e + 1) % 4]
        out = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            dp = (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax)
            dq = (bx - ax) * (q[1] - ay) - (by - ay) * (q[0] - ax)
            if dp >= 0:
                out.append(p)
            if (dp >= 0) != (dq >= 0):
                t = dp / (dp - dq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = out
        if not poly:
            return 0.0
    if len(poly) < 3:
        return 0.0
    return 0.5 * abs(sum(p[0] * q[1] - p[1] * q[0] for p, q in zip(poly, poly[1:] + poly[:1])))


def iou_pair(a, b):
    """(BEV, 3-D) IoU of two boxes [x,y,z,l,w,h,yaw], float64."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    area_a, area_b = a[3] * a[4], b[3] * b[4]
    if not (area_a > 0 and area_b > 0):
        return 0.0, 0.0
    area = _clip_area(_corners(a), _corners(b))
    bev = area / (area_a + area_b - area) if area_a + area_b - area > 0 else 0.0
    dz = max(0.0, min(a[2] + a[5] / 2, b[2] + b[5] / 2) - max(a[2] - a[5] / 2, b[2] - b[5] / 2))
    vol_a, vol_b, inter = area_a * a[5], area_b * b[5], area * dz
    full = inter / (vol_a + vol_b - inter) if vol_a > 0 and vol_b > 0 and vol_a + vol_b - inter > 0 else 0.0
    return bev, full


def iou_table(dts, gts) -> np.ndarray:
    out = np.zeros((len(dts), len(gts), 2), np.float32)
    for i, d in enumerate(dts):
        for j, g in enumerate(gts):
            out[i, j] = iou_pair(d, g)
    return out


def weights(iou, threshold) -> np.ndarray:
    """fp32 IoU -> integer weights: min(1000, floor(1000 * iou)) where iou >= threshold (both fp32), else 0."""
    iou = np.asarray(iou, np.float32)
    w = np.minimum(np.floor(np.float32(1000.0) * iou), 1000).astype(np.int64)
    return np.where(iou >= np.float32(threshold), w, 0)


# ----------------------------------------------------------------------------------------------------------------------
# matching: sequential insertion
# ----------------------------------------------------------------------------------------------------------------------
def insert_rows(W):
    """Rows of the integer weight table ``W`` (n, m) inserted in order; yields, after every row, the column of each row so far
    (``NONE`` = unmatched).  One shortest-augmenting-path search per row on the costs ``-W`` with an always-free zero-cost column
    "unmatched" that wins ties; among real columns the lowest wins."""
    W = np.asarray(W, np.int64)
    n, m = W.shape
    u, v = np.zeros(n, np.int64), np.zeros(m, np.int64)
    owner, col_of = np.full(m, NONE, np.int64), np.full(n, NONE, np.int64)
    big = np.int64(1) << 40
    for r in range(n):
        minv, way, used = np.full(m, big, np.int64), np.full(m, START, np.int64), np.zeros(m, bool)
        i0, j0, dmin, dway = r, START, None, START
        for _ in range(m + 1):
            cur = -W[i0] - u[i0] - v
            better = ~used & (cur < minv)
            minv[better], way[better] = cur[better], j0
            if dmin is None or -u[i0] < dmin:
                dmin, dway = -u[i0], j0
            free = np.flatnonzero(~used)
            j1, delta = NONE, dmin
            if len(free):
                j = free[np.argmin(minv[free])]  # (the first minimum: the lowest column)
                if minv[j] < dmin:
                    j1, delta = int(j), minv[j]
            u[r] += delta
            u[owner[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            dmin -= delta
            if j1 == NONE:
                break
            used[j1] = True
            if owner[j1] < 0:
                break
            j0, i0 = j1, owner[j1]
        else:
            raise AssertionError("a search visits every column at most once")
        target, jc = (j1, way[j1]) if j1 != NONE else (NONE, dway)
        while True:
            rr = r if jc == START else owner[jc]
            col_of[rr] = target
            if target >= 0:
                owner[target] = rr
            if jc == START:
                break
            target, jc = jc, way[jc]
        yield col_of[:r + 1].copy()


def heading_quanta(yaw_d, yaw_g) -> int:
    d = math.fmod(abs(float(np.float32(yaw_d)) - float(np.float32(yaw_g))), 2.0 * math.pi)
    if d > math.pi:
        d = 2.0 * math.pi - d
    acc = 1.0 - d / math.pi
    return int(np.rint(acc * QUANTUM)) if acc >= 0.0 else 0


# ----------------------------------------------------------------------------------------------------------------------
# counts
# ----------------------------------------------------------------------------------------------------------------------
def segment_orders(scene):
    """Per (sweep, type): detection rows by descending score (ties in input order), ground-truth rows in input order."""
    out = {}
    by_score = np.argsort(-np.asarray(scene["scores"], np.float32), kind="stable")
    for s in range(scene["n_sweeps"]):
        for t in range(1, 5):
            d = by_score[(scene["dt_sweep"][by_score] == s) & (scene["dt_type"][by_score] == t)]
            g = np.flatnonzero((scene["gt_sweep"] == s) & (scene["gt_type"] == t))
            out[(s, t)] = (d, g)
    return out


def count_tables(scene, iou=None, thresholds=THRESHOLDS) -> np.ndarray:
    """(2, 16, 2, 101, 4) int64 [TP, FP, FN, heading].  ``scene``: ``dts`` (N,7) f32, ``scores``, ``dt_sweep``, ``dt_type`` (1..4), ``gts``
    (M,7), ``gt_level`` (0 = dropped), ``gt_sweep``, ``gt_type``, ``n_sweeps``.  ``iou``: {(sweep, type): (nd, ng, 2) f32 in segment
    order} or None (float64 clipping, rounded to fp32)."""
    T = np.zeros((2, N_BROWS, 2, N_CUT, 4), np.int64)
    dts, gts, level = np.asarray(scene["dts"], np.float32), np.asarray(scene["gts"], np.float32), np.asarray(scene["gt_level"])
    for (s, t), (d, g) in segment_orders(scene).items():
        if not np.any(level[scene["gt_sweep"] == s] != 0):
            continue  # no ground truth left in the sweep: not a frame
        table = iou_table(dts[d], gts[g]) if iou is None else np.asarray(iou[(s, t)], np.float32).reshape(len(d), len(g), 2)
        ks = np.asarray([cutoff_index(scene["scores"][i]) for i in d], np.int64)
        d_shard = np.asarray([range_shard(dts[i]) for i in d], np.int64)
        g_shard = np.asarray([range_shard(gts[j]) for j in g], np.int64)
        for box in range(2):
            for shard in range(4):
                rows = np.flatnonzero((ks >= 0) & ((d_shard == shard) | (shard == 0)))
                cols = np.flatnonzero((level[g] != 0) & ((g_shard == shard) | (shard == 0)))
                brow = t - 1 if shard == 0 else 4 + (t - 1) * 3 + shard - 1
                W = weights(table[np.ix_(rows, cols)][:, :, box], thresholds[t]) if len(rows) and len(cols) else np.zeros((len(rows), len(cols)), np.int64)
                states = list(insert_rows(W))
                lv = level[g][cols]
                counts = {}  # rows inserted -> the four counts at level 1, 2
                for k in range(N_CUT):
                    n_in = int(np.sum(ks[rows] >= k))  # (score order: the first n_in rows)
                    if n_in not in counts:
                        match = states[n_in - 1] if n_in else np.zeros(0, np.int64)
                        pairs = [(r, c) for r, c in enumerate(match) if c >= 0]
                        assert all(W[r, c] > 0 for r, c in pairs), "a pair of weight 0 is no match"
                        counts[n_in] = []
                        for L in (1, 2):
                            tps = [(r, c) for r, c in pairs if lv[c] <= L]
                            counts[n_in].append((len(tps), n_in - len(pairs), int(np.sum(lv <= L)) - len(tps),
                                                 sum(heading_quanta(dts[d[rows[r]], 6], gts[g[cols[c]], 6]) for r, c in tps)))
                    T[box, brow, :, k] += np.asarray(counts[n_in], np.int64)
    return T


# ----------------------------------------------------------------------------------------------------------------------
# AP / APH
# ----------------------------------------------------------------------------------------------------------------------
def result_row(row: int):
    """Result row 0 .. 31 -> (breakdown row, level index)."""
    return (row // 2 if row < 8 else 4 + (row - 8) // 2), row % 2


def summarize(T) -> np.ndarray:
    out = np.zeros((2, N_RROWS, 2))
    for box in range(2):
        for row in range(N_RROWS):
            brow, lv = result_row(row)
            tp, fp, fn, hd = (T[box, brow, lv, :, i].astype(np.float64) for i in range(4))
            hd = hd / QUANTUM
            for m, num in enumerate((tp, hd)):
                with np.errstate(invalid="ignore", divide="ignore"):
                    p = np.where(tp + fp > 0, num / (tp + fp), 0.0)
                    r = np.where(tp + fn > 0, num / (tp + fn), 0.0)
                p = np.maximum.accumulate(p)  # from the lowest cutoff (highest recall) upwards
                area, before = 0.0, 0.0
                for k in range(N_CUT - 1, -1, -1):
                    area += (r[k] - before) * p[k]
                    before = r[k]
                out[box, row, m] = area
    return out


def layout():
    """The 128 (metric_name, type, category, level, r_lower, r_upper) rows, written out the long way."""
    inf = math.inf
    rows = []
    for metric in ("AP", "APH"):
        for box in ("BEV", "3D"):
            for cat in ("VEHICLE", "PEDESTRIAN", "SIGN", "CYCLIST"):
                rows += [(metric, box, cat, 1, 0.0, inf), (metric, box, cat, 2, 0.0, inf)]
            for cat in ("VEHICLE", "PEDESTRIAN", "SIGN", "CYCLIST"):
                rows += [(metric, box, cat, 1, 0.0, 30.0), (metric, box, cat, 2, 0.0, 30.0), (metric, box, cat, 1, 30.0, 50.0),
                         (metric, box, cat, 2, 30.0, 50.0), (metric, box, cat, 1, 50.0, inf), (metric, box, cat, 2, 50.0, inf)]
    return rows


# ----------------------------------------------------------------------------------------------------------------------
# hand-worked cases
# ----------------------------------------------------------------------------------------------------------------------
def load_cases():
    """``tests/golden/waymo_eval_cases.json`` -> scenes.  A detection is ``[x, y, z, l, w, h, yaw, score, category, sweep]``, a ground
    truth ``[x, y, z, l, w, h, yaw, category, num_interior_pts, difficulty_level, sweep]``; boxes go through the quaternion rows, as
    they do in the evaluator."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "waymo_eval_cases.json")
    cases = []
    for case in json.load(open(path))["cases"]:
        d, g = case["dts"], case["gts"]
        dt_rows = rows_from_yaw([r[:7] for r in d]) if d else np.zeros((0, 10), np.float32)
        gt_rows = rows_from_yaw([r[:7] for r in g]) if g else np.zeros((0, 10), np.float32)
        scene = {"name": case["name"], "n_sweeps": case["n_sweeps"], "expect": case["expect"],
                 "dt_rows": dt_rows, "gt_rows": gt_rows, "dts": boxes_from_rows(dt_rows), "gts": boxes_from_rows(gt_rows),
                 "scores": np.asarray([r[7] for r in d], np.float32), "dt_type": np.asarray([TYPES[r[8]] for r in d], np.int64),
                 "dt_sweep": np.asarray([r[9] for r in d], np.int64), "gt_type": np.asarray([TYPES[r[7]] for r in g], np.int64),
                 "gt_npts": np.asarray([r[8] for r in g], np.int64), "gt_difficulty": np.asarray([r[9] for r in g], np.int64),
                 "gt_sweep": np.asarray([r[10] for r in g], np.int64)}
        scene["gt_level"] = np.asarray([level_of(n, dl) for n, dl in zip(scene["gt_npts"], scene["gt_difficulty"])], np.uint8)
        cases.append(scene)
    return cases


def check_case(case, T, values, tol=1e-6):
    """Counts ``T`` (2,16,2,101,4) and values (2,32,2) against the case's expectations: every listed count over its cutoff span, every
    listed AP / APH, and 0 for every result row the case does not list."""
    shard_of = {"all": 0, "0-30": 1, "30-50": 2, "50-inf": 3}
    for e in case["expect"]["counts"]:
        t = TYPES[e["category"]]
        for box in e["type"]:
            for rng in e["range"]:
                s = shard_of[rng]
                brow = t - 1 if s == 0 else 4 + (t - 1) * 3 + s - 1
                for lv in e["level"]:
                    got = T[("BEV", "3D").index(box), brow, lv - 1, e["k"][0]:e["k"][1] + 1, :3]
                    assert np.all(got == np.asarray([e["TP"], e["FP"], e["FN"]])), (case["name"], e, got)
    listed = np.zeros((2, N_RROWS), bool)
    for e in case["expect"]["values"]:
        t = TYPES[e["category"]]
        for box in e["type"]:
            for rng in e["range"]:
                s = shard_of[rng]
                for lv in e["level"]:
                    row = (t - 1) * 2 + lv - 1 if s == 0 else 8 + (t - 1) * 6 + (s - 1) * 2 + lv - 1
                    b = ("BEV", "3D").index(box)
                    listed[b, row] = True
                    assert abs(values[b, row, 0] - e["AP"]) <= tol and abs(values[b, row, 1] - e["APH"]) <= tol, (case["name"], e, values[b, row])
    assert np.all(values[~listed] == 0.0), (case["name"], "rows the case does not list must be 0", np.argwhere((values != 0).any(-1) & ~listed))
