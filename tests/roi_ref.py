"""NumPy restatement of the declared ROI semantics (include/rv3d.h): the raster lookup of ego-frame points, the box
vertices, the polygon fill, the dilation and the ROI-aware matcher (which wraps ``tests/eval_ref.py``).  Written from the declaration,
in its expression order, in float64; the tests compare ``rv_roi_points`` / ``rv_roi_boxes`` / ``rv_roi_rasterize`` /
``rv_eval_match_roi`` against it bit for bit, and it against the hand-worked cases of ``tests/golden/roi_cases.json``.

A layer is ``(array (height, width), (s, tx, ty))``; a pose is the (3, 4) ``city_SE3_ego``.
"""

from __future__ import annotations

import json
import os

import numpy as np

import eval_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sweep_of_rows(offsets, n: int) -> np.ndarray:
    """CSR offsets (B + 1) -> the sweep of each of the n rows, -1 for a row outside [offsets[0], offsets[B])."""
    off = np.asarray(offsets, np.int64)
    i = np.arange(n, dtype=np.int64)
    sweep = np.searchsorted(off, i, side="right") - 1  # the last sweep whose offset is <= i
    return np.where((i >= off[0]) & (i < off[-1]), np.minimum(sweep, len(off) - 2), -1)


def lookup_ref(xyz, sweep, layer_index, poses, layers):
    """Flags (n,) uint8 of ego-frame points and the number of stray rows (``sweep`` outside [0, B))."""
    p = np.asarray(xyz).astype(np.float64).reshape(-1, 3)
    sweep, layer_index = np.asarray(sweep, np.int64), np.asarray(layer_index, np.int64)
    poses = np.asarray(poses, np.float64).reshape(len(layer_index), 3, 4)
    out = np.zeros(len(p), np.uint8)
    for b in range(len(layer_index)):
        if not 0 <= layer_index[b] < len(layers):
            continue
        rows = np.nonzero(sweep == b)[0]
        arr, (s, tx, ty) = layers[int(layer_index[b])]
        arr, T = np.asarray(arr), poses[b]
        x, y, z = p[rows, 0], p[rows, 1], p[rows, 2]
        with np.errstate(invalid="ignore", over="ignore"):
            pcx = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
            pcy = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
            a, c = (pcx + float(tx)) * float(s), (pcy + float(ty)) * float(s)
            ok = (a > -1.0) & (a < arr.shape[1]) & (c > -1.0) & (c < arr.shape[0])  # false for NaN: nothing non-finite is cast
        u, v = a[ok].astype(np.int64), c[ok].astype(np.int64)  # truncation toward zero
        out[rows[ok]] = arr[v, u] != 0
    return out, int(np.sum((sweep < 0) | (sweep >= len(layer_index))))


def box_vertices_ref(boxes) -> np.ndarray:
    """(n, 10) f32 rows -> (n, 8, 3) f64 vertices ``c + R(q) (+-l/2, +-w/2, +-h/2)``, R of the quaternion as given."""
    r = np.asarray(boxes, np.float32).reshape(-1, 10).astype(np.float64)
    qw, qx, qy, qz = r[:, 6], r[:, 7], r[:, 8], r[:, 9]
    R = [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)],
         [2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)],
         [2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)]]
    half = 0.5 * r[:, 3:6]
    out = np.zeros((len(r), 8, 3))
    for k in range(8):
        d = [half[:, 0] * (-1.0 if k & 4 else 1.0), half[:, 1] * (-1.0 if k & 2 else 1.0), half[:, 2] * (-1.0 if k & 1 else 1.0)]
        for i in range(3):
            out[:, k, i] = r[:, i] + ((R[i][0] * d[0] + R[i][1] * d[1]) + R[i][2] * d[2])
    return out


def boxes_ref(boxes, sweep, layer_index, poses, layers):
    """A box is inside iff any of its 8 vertices is.  Flags (n,) uint8 and the number of stray rows."""
    verts = box_vertices_ref(boxes)
    n = len(verts)
    flags, stray = lookup_ref(verts.reshape(-1, 3), np.repeat(np.asarray(sweep, np.int64), 8), layer_index, poses, layers)
    return flags.reshape(n, 8).max(1) if n else np.zeros(0, np.uint8), stray // 8


def fill_ref(polygons, s, tx, ty, height, width) -> np.ndarray:
    """Pixel (v, u) is drivable iff its centre (u + 0.5, v + 0.5) is inside any polygon by the even-odd rule."""
    cx, cy = (np.arange(width) + 0.5)[None, :], (np.arange(height) + 0.5)[:, None]
    out = np.zeros((height, width), bool)
    for poly in polygons:
        p = np.asarray(poly, np.float64).reshape(-1, 2)
        px, py = (p[:, 0] + float(tx)) * float(s), (p[:, 1] + float(ty)) * float(s)
        crossings = np.zeros((height, width), np.int64)
        for i in range(len(p)):
            k = (i + 1) % len(p)
            ax, ay, bx, by = px[i], py[i], px[k], py[k]
            with np.errstate(divide="ignore", invalid="ignore"):
                x_at = ax + (cy - ay) * (bx - ax) / (by - ay)
                crossings += ((ay <= cy) != (by <= cy)) & (x_at > cx)
        out |= (crossings & 1) != 0
    return out.astype(np.uint8)


def dilate_ref(drivable, r: float) -> np.ndarray:
    """A pixel is ROI iff some drivable pixel lies at an integer offset (du, dv) with du^2 + dv^2 <= r^2 (outside the image: nothing)."""
    d = np.asarray(drivable) != 0
    h, w = d.shape
    out = np.zeros_like(d)
    reach = int(np.floor(r))
    for dv in range(-reach, reach + 1):
        for du in range(-reach, reach + 1):
            if float(du * du + dv * dv) > float(r) * float(r) or abs(dv) >= h or abs(du) >= w:
                continue
            # out[v, u] |= d[v + dv, u + du]
            out[max(0, -dv):h - max(0, dv), max(0, -du):w - max(0, du)] |= d[max(0, dv):h - max(0, -dv), max(0, du):w - max(0, -du)]
    return out.astype(np.uint8)


def match_roi_ref(dts, scores, dt_sweep, dt_cat, dt_roi, gts, gt_valid, gt_roi, gt_sweep, gt_cat, n_sweeps, n_cat, cfg):
    """The ROI-aware matcher: per segment the rows in range, in score order, the first ``max_num_dts_per_category`` of them (whatever
    their flag) and of those the flagged ones are evaluated; ground truth needs its flag too.  The evaluated rows then go through
    ``eval_ref.match_ref`` (at most the cap per segment and all in range, so its own two filters keep every one of them)."""
    dts, scores = np.asarray(dts, np.float32).reshape(-1, 10), np.asarray(scores, np.float32)
    dt_sweep, dt_cat, dt_roi = np.asarray(dt_sweep), np.asarray(dt_cat), np.asarray(dt_roi)
    n, n_thr = len(dts), len(cfg.affinity_thresholds_m)
    r2 = float(cfg.max_range_m) * float(cfg.max_range_m)
    keep = []
    for s in range(n_sweeps):
        for c in range(n_cat):
            rows = np.nonzero((dt_sweep == s) & (dt_cat == c))[0]
            rows = rows[eval_ref._norm2(dts[rows, :3]) <= r2]
            rows = rows[np.argsort(-scores[rows], kind="stable")][: cfg.max_num_dts_per_category]  # the cap first ...
            keep.extend(rows[dt_roi[rows] != 0].tolist())  # ... then the ROI flag
    keep = np.sort(np.asarray(keep, np.int64))  # input order: ties keep their order in match_ref's stable sort
    valid = (np.asarray(gt_roi) != 0) & (np.ones(len(np.asarray(gts).reshape(-1, 10)), bool) if gt_valid is None else np.asarray(gt_valid) != 0)
    sub = eval_ref.match_ref(dts[keep], scores[keep], dt_sweep[keep], dt_cat[keep], gts, valid, gt_sweep, gt_cat, n_sweeps, n_cat, cfg)
    out = {"evaluated": np.zeros(n, np.uint8), "tp": np.zeros((n, n_thr), np.uint8), "err": np.full((n, 3), np.nan),
           "matched_gt": np.full(n, -1, np.int32), "gt_evaluated": sub["gt_evaluated"]}
    for key in ("evaluated", "tp", "err", "matched_gt"):
        out[key][keep] = sub[key]
    return out


def _number(v) -> float:
    return float(v)  # "nan" / "inf" are spelled as strings in the JSON file


def load_cases():
    """``tests/golden/roi_cases.json`` as arrays: ``layers`` [(array, (s, tx, ty))], ``layer_index`` (B,), ``poses`` (B, 3, 4), ``points``
    {xyz (n, 3) f64, sweep, expect, why}, ``boxes`` {rows (n, 10) f32, sweep, expect, why}, ``match`` (the cap-rule scene)."""
    raw = json.load(open(os.path.join(GOLDEN, "roi_cases.json")))
    layers = [(np.asarray(l["array"], np.uint8), (float(l["s"]), float(l["tx"]), float(l["ty"]))) for l in raw["layers"]]
    pts, boxes = raw["points"], raw["boxes"]
    return {"layers": layers, "layer_names": [l["name"] for l in raw["layers"]],
            "layer_index": np.asarray([s["layer"] for s in raw["sweeps"]], np.int64),
            "poses": np.asarray([s["city_SE3_ego"] for s in raw["sweeps"]], np.float64).reshape(-1, 3, 4),
            "points": {"xyz": np.asarray([[_number(v) for v in p["xyz"]] for p in pts], np.float64), "sweep": np.asarray([p["sweep"] for p in pts], np.int64),
                       "expect": np.asarray([p["expect"] for p in pts], np.uint8), "why": [p["why"] for p in pts]},
            "boxes": {"rows": np.asarray([b["row"] for b in boxes], np.float32), "sweep": np.asarray([b["sweep"] for b in boxes], np.int64),
                      "expect": np.asarray([b["expect"] for b in boxes], np.uint8), "why": [b["why"] for b in boxes]},
            "match": raw["match"]}


# the issue's polygons for the fill / dilation checks: a concave pentagon and a triangle, s = 1, t = (2, 3), raster 80 x 96
POLYGONS = [[(3.2, 4.1), (40.7, 6.3), (38.9, 30.2), (22.4, 18.8), (5.6, 33.3)], [(50.3, 40.2), (70.1, 41.7), (60.4, 55.9)]]
POLYGON_RASTER = {"s": 1.0, "tx": 2.0, "ty": 3.0, "height": 80, "width": 96}
