"""The accuracy of the rotated IoU of ``csrc/nms_geom.h`` on the device, through every entry that returns an IoU or decides by one,
against the independent float64 reference and the error bound of ``tests/iou_ref.py``: pair families at 0, 30, 75 and 200 m (cars,
pedestrians, long near-parallel trucks, identical boxes, shared edges, touching corners, containment, concentric turns, thin boxes,
boxes without area, pairs at the edge of the bounding-circle exits).  ``tests/test_iou_ref_cpu.py`` holds the CPU half: the
reference against closed forms, and the same arithmetic on the CPU within the same bound.

Every family is 120 pairs; the dense entries see the 120 x 120 table of a family (the pairs are its diagonal; off the diagonal the
boxes are mostly metres apart, which is what the exits are for).  The whole file takes a few seconds."""

from __future__ import annotations

import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import iou_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))  # (a copy: the arrays of a case are read-only)
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the entries ---------------------------------------------------------------------------------------------------------------------
def rotated_iou(ra, rb) -> np.ndarray:
    """``rv_rotated_iou``: (n,5) x (m,5) rectangles -> (n,m)."""
    from range_view_3d_detection_amd import _lib as L

    a, b = _dev(ra, torch.float32), _dev(rb, torch.float32)
    out = torch.full((a.shape[0], b.shape[0]), float("nan"), dtype=torch.float32, device=DEV)
    L.call("rv_rotated_iou", L.ptr(a), a.shape[0], L.ptr(b), b.shape[0], L.ptr(out), L.stream_ptr())
    return out.cpu().numpy()


def mmcv_iou(a7, b7, aligned) -> np.ndarray:
    from range_view_3d_detection_amd.compat.mmcv_ops import box_iou_rotated

    return box_iou_rotated(_dev(R.mmcv_of(a7)), _dev(R.mmcv_of(b7)), aligned=aligned).cpu().numpy()


def iou3d(a7, b7) -> np.ndarray:
    from range_view_3d_detection_amd.compat.mmcv_ops import boxes_iou3d

    return boxes_iou3d(_dev(a7), _dev(b7)).cpu().numpy()


def waymo_iou(a7, b7) -> np.ndarray:
    """``rv_waymo_iou`` on one segment: (n,7) detections x (m,7) ground truth -> (n,m,2) [BEV, 3-D]."""
    from range_view_3d_detection_amd.evaluation import waymo as W

    n, m = len(a7), len(b7)
    ws = W.pairwise_iou(_dev(a7), _dev(np.arange(n)), _dev(np.asarray([0, n])), _dev(b7), _dev(np.arange(m)), _dev(np.asarray([0, m])), 1)
    _, table = W._workspace_views(ws, 1)
    return table[:n * m].reshape(n, m, 2).cpu().numpy()


_TABLES = {}


def tables(family, dist):
    """Every entry on one case, computed once: name -> (values of the pairs (n,), is it the 3-D IoU, the dense table or None)."""
    key = (family, dist)
    if key not in _TABLES:
        c = R.case(family, dist)
        dense, dense_mmcv, dense_3d, way = rotated_iou(c.ra, c.rb), mmcv_iou(c.a, c.b, False), iou3d(c.a, c.b), waymo_iou(c.a, c.b)
        _TABLES[key] = {"rv_rotated_iou": (dense.diagonal(), False, dense),
                        "box_iou_rotated aligned": (mmcv_iou(c.a, c.b, True), False, None),
                        "box_iou_rotated dense": (dense_mmcv.diagonal(), False, dense_mmcv),
                        "boxes_iou3d": (dense_3d.diagonal(), True, dense_3d),
                        "rv_waymo_iou BEV": (way[:, :, 0].diagonal(), False, way[:, :, 0]),
                        "rv_waymo_iou 3-D": (way[:, :, 1].diagonal(), True, way[:, :, 1])}
    return _TABLES[key]


# ---- values ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_every_entry_is_within_tol_of_the_float64_reference(family):
    """``|device - iou64| <= tol`` and ``|device3d - iou3d64| <= tol3d`` pair by pair, ``0 <= device <= 1 + tol``, identical pairs within
    ``tol`` of 1, pairs without area exactly 0, ``circle_margin`` pairs exactly 0 outside the circle and not lost inside it
    (``iou_ref.check_values``).  Prints the worst ``error / tol`` of the family per distance."""
    worst = {}
    for d in R.DISTANCES:
        c = R.case(family, d)
        for name, (values, three_d, _) in tables(family, d).items():
            assert values.shape == (len(c.a),) and values.dtype == np.float32 and np.isfinite(values).all(), name
            worst.setdefault(d, []).append(R.check_values(c, values, name, three_d))
    print(f"device {family}: worst error / tol at {R.DISTANCES} m: " + ", ".join(f"{max(worst[d]):.3f}" for d in R.DISTANCES))


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_entries_that_share_the_arithmetic_are_bit_identical(family):
    """``rv_rotated_iou``, ``rv_rotated_iou_pairs`` and the BEV column of ``rv_waymo_iou`` (whose bounding-circle exit must change no
    bit: the whole 120 x 120 table, near pairs and far); ``rv_boxes_iou3d`` and the 3-D column of ``rv_waymo_iou``."""
    for d in R.DISTANCES:
        t = tables(family, d)
        dense = t["rv_rotated_iou"][2]
        assert np.array_equal(_bits(dense), _bits(t["box_iou_rotated dense"][2])), (family, d)
        assert np.array_equal(_bits(dense), _bits(t["rv_waymo_iou BEV"][2])), (family, d, "the exit of waymo_iou_pair changed a value")
        assert np.array_equal(_bits(dense.diagonal()), _bits(t["box_iou_rotated aligned"][0])), (family, d)
        assert np.array_equal(_bits(t["boxes_iou3d"][2]), _bits(t["rv_waymo_iou 3-D"][2])), (family, d)
        # off the diagonal too the table is an IoU: none above what the largest bound of the case allows
        assert dense.min() >= 0.0 and dense.max() <= 1.0 + R.case(family, d).tol.max()


def test_the_clip_of_a_box_by_itself_returns_its_own_corners():
    """Identical pairs, bit for bit against ``iou_ref.self_iou32``: closed half-plane tests (``dp >= 0``) interpolate nothing on a box
    clipped by itself.  (Open tests stay within ``tol``; the last bits tell, near the origin.)"""
    for d in R.DISTANCES:
        c = R.case("identical", d)
        assert np.array_equal(_bits(tables("identical", d)["rv_rotated_iou"][0]), _bits(R.self_iou32(c.ra))), d


# ---- shapes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 1), (63, 65), (257, 3), (0, 5)])
def test_shapes(n, m):
    """Row i is pair ``i mod 120`` of the cars at 75 m, column j likewise: element (i, j) with ``i = j (mod 120)`` has a reference."""
    c = R.case("cars", 75.0)
    i, j = np.arange(n) % len(c.a), np.arange(m) % len(c.b)
    dense = rotated_iou(c.ra[i], c.rb[j])
    assert dense.shape == (n, m) and not np.isnan(dense).any()
    assert np.array_equal(_bits(dense), _bits(mmcv_iou(c.a[i], c.b[j], False)))
    flat = mmcv_iou(c.a[i].repeat(m, 0), np.tile(c.b[j], (n, 1)), True)  # every pair of the table through the per-pair kernel
    assert flat.shape == (n * m,) and np.array_equal(_bits(dense.reshape(-1)), _bits(flat))
    way, d3 = waymo_iou(c.a[i], c.b[j]), iou3d(c.a[i], c.b[j])
    assert d3.shape == (n, m) and np.array_equal(_bits(way[:, :, 0]), _bits(dense)) and np.array_equal(_bits(way[:, :, 1]), _bits(d3))
    same = i[:, None] == j[None, :]
    assert same.sum() >= min(n, m)
    want, bound = np.broadcast_to(c.iou[i][:, None], (n, m))[same], np.broadcast_to(c.tol[i][:, None], (n, m))[same]
    assert np.all(np.abs(dense[same] - want) <= bound)
    want3, bound3 = np.broadcast_to(c.iou3d[i][:, None], (n, m))[same], np.broadcast_to(c.tol3d[i][:, None], (n, m))[same]
    assert np.all(np.abs(d3[same] - want3) <= bound3)


def test_grid_stride_loop_runs_twice():
    """1025 x 1024 pairs are more than the 4096 x 256 threads of the launch: the same rows in calls of at most 256 rows, bit for bit."""
    rows = np.concatenate([R.case(f, 75.0).ra for f in sorted(R.FAMILIES)])[:1025]
    cols = np.concatenate([R.case(f, 75.0).rb for f in sorted(R.FAMILIES)])[:1024]
    assert rows.shape == (1025, 5) and cols.shape == (1024, 5) and 1025 * 1024 > 4096 * 256
    whole = rotated_iou(rows, cols)
    parts = np.concatenate([rotated_iou(rows[k:k + 256], cols) for k in range(0, 1025, 256)])
    assert whole.shape == parts.shape == (1025, 1024) and np.array_equal(_bits(whole), _bits(parts))
    assert (whole > 0.1).sum() >= 500 and not np.isnan(whole).any()


# ---- decisions -------------------------------------------------------------------------------------------------------------------------
def _decided(families, dist, threshold, three_d=False, limit=8):
    """Pairs whose exact IoU is at least ``2 tol`` above / below the threshold, the ``limit`` closest to it on either side:
    [(case, pair index)], [(case, pair index)]."""
    above, below = [], []
    for f in families:
        c = R.case(f, dist)
        v, t = (c.iou3d, c.tol3d) if three_d else (c.iou, c.tol)
        above += [(v[k] - threshold, c, k) for k in np.flatnonzero(v >= threshold + 2 * t)]
        below += [(threshold - v[k], c, k) for k in np.flatnonzero((v <= threshold - 2 * t) & (v > 0.05))]
    pick = lambda rows: [(c, int(k)) for _, c, k in sorted(rows, key=lambda r: r[0])[:limit]]  # noqa: E731
    above, below = pick(above), pick(below)
    assert len(above) == limit and len(below) == limit, (dist, threshold, len(above), len(below))
    return above, below


NMS_FAMILIES = ("cars", "pedestrians", "thin")


@pytest.mark.parametrize("dist", [75.0, 200.0])
def test_weighted_nms_on_two_box_lists(dist):
    """``math.ops.nms.weighted_nms`` (nms.hip; merge threshold = NMS threshold = 0.3): one row of count 2 above, two rows below."""
    from range_view_3d_detection_amd.math.ops import nms as hnms

    scores = _dev(np.asarray([0.9, 0.8], np.float32))
    for side, pairs in zip(("above", "below"), _decided(NMS_FAMILIES, dist, 0.3)):
        for c, k in pairs:
            rect = _dev(np.stack([c.ra[k], c.rb[k]]))
            keep, rows, count = hnms.weighted_nms(rect, rect[:, :4].contiguous(), scores, 0.3, 0.3)
            want = ([0], [2]) if side == "above" else ([0, 1], [1, 1])
            assert (keep.tolist(), count.tolist()) == want and rows.shape[0] == len(want[0]), (c.family, dist, k, c.iou[k], side)


@pytest.mark.parametrize("dist", [75.0, 200.0])
def test_nms_rotated_on_two_box_lists(dist):
    """``compat.detectron2_nms.nms_rotated`` takes degrees, clockwise: the rectangle it hands the kernel has the yaw
    ``fp32(-deg * pi / 180)``, which is not the yaw of the pair -- the pair is judged by the reference ON THAT rectangle."""
    from range_view_3d_detection_amd.compat.detectron2_nms import nms_rotated

    scores = _dev(np.asarray([0.9, 0.8], np.float32))
    done = {"above": 0, "below": 0}
    for side, pairs in zip(("above", "below"), _decided(NMS_FAMILIES, dist, 0.3)):
        for c, k in pairs:
            boxes = np.stack([R.mmcv_of(c.a[k:k + 1])[0], R.mmcv_of(c.b[k:k + 1])[0]])
            boxes[:, 4] = (-boxes[:, 4].astype(np.float64) * 180.0 / math.pi).astype(np.float32)
            handed = np.stack([c.ra[k], c.rb[k]])
            handed[:, 4] = (torch.from_numpy(boxes[:, 4:5].copy()) * (-math.pi / 180.0)).numpy()[:, 0]
            exact, bound = R.iou64(handed[0], handed[1]), R.tol(handed[0], handed[1])
            if abs(exact - 0.3) < 2 * bound or (exact > 0.3) != (side == "above"):
                continue  # (the change of the yaw moved the pair into the band around the threshold)
            kept = nms_rotated(_dev(boxes), scores, torch.as_tensor(0.3)).tolist()
            assert kept == ([0] if side == "above" else [0, 1]), (c.family, dist, k, exact, side)
            done[side] += 1
    assert min(done.values()) >= 6, done


@pytest.mark.parametrize("mode", ["WEIGHTED", "HARD"])
@pytest.mark.parametrize("dist", [75.0, 200.0])
def test_batched_multiclass_nms_on_two_sweeps_of_two_boxes(dist, mode):
    """``batched_multiclass_nms`` (nms2.hip): sweep 0 holds a pair above 0.3, sweep 1 a pair below: 1 row and 2 rows."""
    from range_view_3d_detection_amd.math.ops import nms as hnms

    above, below = _decided(NMS_FAMILIES, dist, 0.3)
    scores, cats = _dev(np.asarray([[0.9, 0.8], [0.9, 0.8]], np.float32)), _dev(np.zeros((2, 2), np.int64))
    for (ca, ka), (cb, kb) in zip(above, below):
        cub = _dev(np.stack([np.stack([ca.a[ka], ca.b[ka]]), np.stack([cb.a[kb], cb.b[kb]])]))
        boxes, sc, _, ids = hnms.batched_multiclass_nms(cub, scores, cats, 100, 100, 0.3, 0.1, mode, n_classes=1)
        assert ids.tolist() == [0.0, 1.0, 1.0] and boxes.shape == (3, 7), (mode, dist, ca.family, ka, ca.iou[ka], cb.family, kb, cb.iou[kb])
        if mode == "HARD":  # rows are input rows
            assert torch.equal(boxes, torch.cat([cub[0, :1], cub[1]])) and sc.tolist() == [np.float32(0.9), np.float32(0.9), np.float32(0.8)]


@pytest.mark.parametrize("dist", [75.0, 200.0])
@pytest.mark.parametrize("family,obj_type,threshold", [("cars", 1, 0.7), ("pedestrians", 2, 0.5)])
def test_waymo_match_on_one_detection_and_one_ground_truth(family, obj_type, threshold, dist):
    """``rv_waymo_iou`` + ``rv_waymo_match`` through ``evaluation.waymo.accumulate``: every sweep holds one detection and one ground-truth
    box of the type; above the type's threshold the sweep is a TP, below it an FP and an FN -- per box type (BEV / 3-D), with the
    pairs chosen by that box type's exact IoU."""
    from range_view_3d_detection_amd.evaluation import waymo as W

    for box, three_d in ((0, False), (1, True)):
        for side, pairs in zip(("above", "below"), _decided((family,), dist, threshold, three_d)):
            n = len(pairs)
            dts, gts = np.stack([c.a[k] for c, k in pairs]), np.stack([c.b[k] for c, k in pairs])
            segment = _dev(np.arange(n, dtype=np.int64) * 4 + obj_type - 1)
            tables = torch.zeros(W.TABLE_SHAPE, dtype=torch.int64, device=DEV)
            errors = torch.zeros(4, dtype=torch.int32, device=DEV)
            W.accumulate(_dev(dts), _dev(np.ones(n, np.float32)), segment, _dev(gts), _dev(np.ones(n, np.uint8)), segment, n,
                         W.WaymoDetectionCfg(), tables, errors)
            assert errors.tolist() == [0, 0, 0, 0]
            got = tables[box, obj_type - 1, :, :, :3].cpu().numpy()  # (level, cutoff, [TP, FP, FN]): score 1 is in at every cutoff
            want = [n, 0, 0] if side == "above" else [0, n, n]
            assert np.all(got == np.asarray(want)), (family, dist, ("BEV", "3-D")[box], side, got[0, 0].tolist(), want)


# ---- the BEV affinity of soft assignment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["cars", "pedestrians"])
def test_bev_affinity_of_soft_assignment(family):
    """``rv_soft_assign`` (softassign.hip) with one level, one task, BEV, ``normalize_affinities`` off and ``k = inf`` leaves the raw
    affinity of every foreground pixel in its map: the clamped IoU of the box decoded from the pixel's regressands and the box decoded
    from its regression targets.  One sweep of one row; pixel k sits at the centre of the second box of pair k of the family at 75 m and
    is its own instance; the regressands encode the first box, the targets the second.  The kernel is handed the DECODED fp32 boxes
    (``oracle.decode.decode_range_view`` restates the decode: fp64, rounded to fp32) and forms ``x -+ l/2`` in fp32: the reference is
    evaluated on exactly those rectangles.  (Where the device's decode rounds a box one fp32 step away from the restatement's, the IoU
    moves by the order of 1e-7: a hundredth of ``tol`` at 75 m.)"""
    from oracle.decode import decode_range_view
    from test_gpu_assignment import INF, _Table

    c = R.case(family, 75.0)
    n = len(c.a)
    a, b = c.a.astype(np.float64), c.b.astype(np.float64)
    az = np.arctan2(b[:, 1], b[:, 0])

    def encode(box):  # azimuth-invariant coding about the pixel at the centre of b
        dx, dy = box[:, 0] - b[:, 0], box[:, 1] - b[:, 1]
        rows = [np.cos(az) * dx + np.sin(az) * dy, np.cos(az) * dy - np.sin(az) * dx, box[:, 2] - b[:, 2], np.log(box[:, 3]), np.log(box[:, 4]),
                np.log(box[:, 5]), np.sin(box[:, 6] - az), np.cos(box[:, 6] - az)]
        return torch.from_numpy(np.stack(rows)).float().view(1, 8, 1, n)

    cart = torch.from_numpy(np.ascontiguousarray(b[:, :3].T)).float().view(1, 3, 1, n)
    reg, tgt = encode(a), encode(b)
    targets = {"panoptics": torch.arange(1, n + 1).view(1, 1, 1, n), "regression_targets": tgt,
               "classification_labels": torch.zeros(1, 1, n, dtype=torch.int64), "points_per_obj": torch.ones(1, 1, 1, n, dtype=torch.int64)}
    e = {"logits": torch.zeros(1, 1, 1, n), "regressands": reg, "cart": cart, "mask": torch.ones(1, 1, 1, n, dtype=torch.bool), "targets": targets}
    t = _Table([e]).assign("BEV", False, INF, torch.tensor([0, n], dtype=torch.int32, device=DEV), n)
    torch.cuda.synchronize()
    got = t.maps[0].flatten().cpu().numpy().astype(np.float64)
    half = np.float32(0.5)
    rects = []
    for coded in (reg, tgt):
        box = decode_range_view(coded, cart, True)[0, :, 0].T.contiguous().numpy()
        assert box.dtype == np.float32 and box.shape == (n, 7)
        rects.append(np.stack([box[:, 0] - half * box[:, 3], box[:, 1] - half * box[:, 4], box[:, 0] + half * box[:, 3], box[:, 1] + half * box[:, 4], box[:, 6]], 1))
    # the decoded rectangles are the family's to well below a millimetre (the yaw to 1e-6 rad: it is unwrapped about the azimuth)
    assert np.abs(rects[0][:, :4] - c.ra[:, :4]).max() < 1e-4 and np.abs(rects[1][:, :4] - c.rb[:, :4]).max() < 1e-4
    assert np.abs(np.sin(0.5 * (rects[0][:, 4].astype(np.float64) - c.ra[:, 4]))).max() < 1e-6
    exact = np.asarray([R.iou64(p, q) for p, q in zip(*rects)])
    bound = np.asarray([R.tol(p, q) for p, q in zip(*rects)])
    err = np.abs(got - exact)
    k = int(np.argmax(err / bound))
    print(f"device soft-assign BEV affinity, {family} at 75 m: worst error / tol {err[k] / bound[k]:.3f}")
    assert np.all(err <= bound), (family, k, got[k], exact[k], bound[k])
    assert exact.min() > 0.1 and np.abs(exact - c.iou).max() < 1e-3  # (the pairs are the family's: real overlaps)
