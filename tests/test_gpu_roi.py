"""AV2 ROI on the device (``rv_roi_points`` / ``rv_roi_boxes`` / ``rv_roi_rasterize`` / ``rv_eval_match_roi``, ``converters.av2.roi``,
the ``roi=`` path of ``evaluation.DetectionEvaluator`` / ``evaluate``) against the hand-worked cases of ``tests/golden/roi_cases.json``
and the NumPy restatement of the declared semantics (``tests/roi_ref.py``).

Bar: every output is a uint8 flag or an integer decided on fp64 arithmetic in the header's expression order, so every comparison
is EXACT; the metric table with an all-covering ROI is bit-identical to the table without the filter.
"""

from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch

import eval_ref
import roi_ref as ref
from test_evaluation_cpu import _cfg
from test_gpu_evaluation import _scene
from test_roi_cpu import CASES, match_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _atlas(layers, names=None):
    from range_view_3d_detection_amd.converters.av2.roi import RoiAtlas

    names = names or [f"log{k}" for k in range(len(layers))]
    return RoiAtlas.from_rasters(names, [l[0] for l in layers], [l[1] for l in layers]).to(DEV)


def _points(xyz, sweep, layer_index, poses, layers, dtype, lead=0, tail=0):
    """Rows grouped by sweep (CSR) through ``roi_points``; ``lead`` / ``tail`` extra rows in front of / behind every sweep (stray).
    Returns the flags in the input order of ``xyz`` and the stray count."""
    from range_view_3d_detection_amd.converters.av2.roi import roi_points

    order = np.argsort(sweep, kind="stable")
    counts = np.bincount(sweep, minlength=len(layer_index))
    offsets = lead + np.concatenate([[0], np.cumsum(counts)])
    rows = np.concatenate([np.zeros((lead, 3)), xyz[order], np.zeros((tail, 3))]).astype(dtype)
    stray = torch.zeros((), dtype=torch.int64, device=DEV)
    got = roi_points(_dev(rows), _dev(offsets.astype(np.int64)), _dev(layer_index), _dev(poses), _atlas(layers), stray=stray).cpu().numpy()
    out = np.empty(len(xyz), np.uint8)
    out[order] = got[lead:lead + len(xyz)]
    assert not got[:lead].any() and not got[lead + len(xyz):].any()
    return out, int(stray)


def _random_layers(g):
    """Two rasters with different sizes, s (1 / 0.3 and 1.0) and t, about half of the cells set."""
    return [((g.random((37, 53)) < 0.5).astype(np.uint8), (1 / 0.3, -100.25, 40.5)), ((g.random((64, 40)) < 0.5).astype(np.uint8), (1.0, 12.0, -7.0))]


def _random_pose(g):
    """A general rigid pose: yaw anywhere, a few degrees of roll and pitch, a translation of some hundred metres."""
    yaw, pitch, roll = g.uniform(-math.pi, math.pi), g.uniform(-0.1, 0.1), g.uniform(-0.1, 0.1)
    cz, sz, cy, sy, cx, sx = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return np.concatenate([R, g.uniform(-300, 300, (3, 1))], 1)


def _ego_points_over(g, n, layer, pose, beyond=4.0):
    """n ego-frame points whose city-frame image is uniform over the layer's extent grown by ``beyond`` cells on every side."""
    arr, (s, tx, ty) = layer
    a, b = g.uniform(-beyond, arr.shape[1] + beyond, n), g.uniform(-beyond, arr.shape[0] + beyond, n)
    city = np.stack([a / s - tx, b / s - ty, g.uniform(-2, 2, n)], 1)
    return (city - pose[:, 3]) @ pose[:, :3]  # R^T (pc - t)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_points_hand_worked_cases(dtype):
    p = CASES["points"]
    got, stray = _points(p["xyz"], p["sweep"], CASES["layer_index"], CASES["poses"], CASES["layers"], dtype)
    assert stray == 0
    wrong = [p["why"][i] for i in np.nonzero(got != p["expect"])[0]]
    assert not wrong, wrong


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("sizes", [(1000, 1, 0), (0, 1, 0, 1000, 0)], ids=["1000-1-0", "empty-first"])
def test_points_against_the_restatement_with_empty_and_one_point_sweeps(dtype, sizes):
    g = np.random.default_rng(np.random.randint(1 << 30))
    layers = _random_layers(g)
    layer_index = np.arange(len(sizes)) % 2
    poses = np.stack([_random_pose(g) for _ in sizes])
    xyz = np.concatenate([_ego_points_over(g, n, layers[layer_index[b]], poses[b]) for b, n in enumerate(sizes)]).astype(dtype)
    sweep = np.repeat(np.arange(len(sizes)), sizes)
    want, _ = ref.lookup_ref(xyz, sweep, layer_index, poses, layers)
    got, stray = _points(xyz, sweep, layer_index, poses, layers, dtype, lead=3, tail=2)
    assert stray == 5 and np.array_equal(got, want)
    assert 0.2 < want.mean() < 0.6


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
def test_points_random_beyond_every_raster_edge(dtype):
    from range_view_3d_detection_amd._lib import RvError
    from range_view_3d_detection_amd.converters.av2.roi import roi_points

    g = np.random.default_rng(np.random.randint(1 << 30))
    layers = _random_layers(g)
    layer_index, poses = np.array([1, 0, 5]), np.stack([_random_pose(g) for _ in range(3)])
    xyz = np.concatenate([_ego_points_over(g, 2048, layers[1], poses[0]), _ego_points_over(g, 2040, layers[0], poses[1]),
                          _ego_points_over(g, 8, layers[0], poses[2])]).astype(dtype)
    sweep = np.repeat([0, 1, 2], [2048, 2040, 8])
    want, _ = ref.lookup_ref(xyz, sweep, layer_index, poses, layers)
    got, stray = _points(xyz, sweep, layer_index, poses, layers, dtype)
    assert stray == 0 and np.array_equal(got, want) and not got[-8:].any()  # (layer index 5 names no layer)
    # points land beyond each of the four edges of both rasters, and inside
    for b in (0, 1):
        arr, (s, tx, ty) = layers[layer_index[b]]
        pc = xyz[sweep == b].astype(np.float64) @ poses[b][:, :3].T + poses[b][:, 3]
        a, c = (pc[:, 0] + tx) * s, (pc[:, 1] + ty) * s
        assert (a < -1).any() and (a > arr.shape[1]).any() and (c < -1).any() and (c > arr.shape[0]).any() and got[sweep == b].sum() > 300
    # without a counter of the caller's the count is read back: rows outside every sweep raise
    with pytest.raises(RvError, match="belong to no sweep"):
        roi_points(_dev(xyz[:10]), _dev(np.array([0, 4, 6, 8])), _dev(layer_index), _dev(poses), _atlas(layers))


def test_boxes_against_the_hand_worked_cases_and_the_restatement():
    from range_view_3d_detection_amd.converters.av2.roi import roi_boxes

    b = CASES["boxes"]
    atlas = _atlas(CASES["layers"])
    got = roi_boxes(_dev(b["rows"]), _dev(b["sweep"]), _dev(CASES["layer_index"]), _dev(CASES["poses"]), atlas).cpu().numpy()
    wrong = [b["why"][i] for i in np.nonzero(got != b["expect"])[0]]
    assert not wrong, wrong
    # 512 boxes with random unit quaternions over 3 sweeps and 2 layers; 5 rows name no sweep
    g = np.random.default_rng(np.random.randint(1 << 30))
    layers = _random_layers(g)
    layer_index, poses = np.array([0, 1, 0]), np.stack([_random_pose(g) for _ in range(3)])
    sweep = g.integers(0, 3, 512)
    centre = np.stack([_ego_points_over(g, 1, layers[layer_index[s]], poses[s], beyond=2.0)[0] for s in sweep])
    q = g.normal(size=(512, 4))
    rows = np.concatenate([centre, g.uniform(0.3, 4, (512, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)], 1).astype(np.float32)
    sweep[[7, 99, 300]], sweep[[8, 511]] = 3, -1
    want, want_stray = ref.boxes_ref(rows, sweep, layer_index, poses, layers)
    stray = torch.zeros((), dtype=torch.int64, device=DEV)
    got = roi_boxes(_dev(rows), _dev(sweep), _dev(layer_index), _dev(poses), _atlas(layers), stray=stray).cpu().numpy()
    assert np.array_equal(got, want) and int(stray) == want_stray == 5
    centre_only, _ = ref.lookup_ref(rows[:, :3], sweep, layer_index, poses, layers)
    assert 0.3 < want.mean() < 0.98 and (want != centre_only).sum() > 30  # the vertices decide, not the centre


STAR = [(30 + (18 if k % 2 else 9 + 0.01 * k) * math.cos(2 * math.pi * k / 700), 28 + (18 if k % 2 else 9 + 0.01 * k) * math.sin(2 * math.pi * k / 700))
        for k in range(700)]  # 700 edges: three LDS chunks


@pytest.mark.parametrize("width,polygons", [(96, ref.POLYGONS), (70, ref.POLYGONS), (70, ref.POLYGONS + [STAR]), (5, [])],
                         ids=["96-wide", "70-wide-clipped", "700-edges", "no-polygon"])
def test_rasterize_against_the_restatement(width, polygons):
    from range_view_3d_detection_amd.converters.av2.roi import rasterize_polygons

    geo = dict(ref.POLYGON_RASTER, width=width)
    want = ref.fill_ref(polygons, geo["s"], geo["tx"], geo["ty"], geo["height"], width)
    if width == 70 and polygons:
        assert want[:, -1].any()  # the triangle is cut by the image edge
    verts = np.asarray([v for p in polygons for v in p], np.float64).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in polygons])]).astype(np.int64)
    for r in (0.0, 5.0, 16.5):
        drivable, roi = rasterize_polygons(_dev(verts), _dev(offsets), geo["s"], geo["tx"], geo["ty"], geo["height"], width, r)
        assert np.array_equal(drivable.cpu().numpy(), want), r
        assert np.array_equal(roi.cpu().numpy(), ref.dilate_ref(want, r)), r
        if r == 0.0:
            assert torch.equal(drivable, roi)
    if width == 96:
        assert int(want.sum()) == 875 and int(roi.sum()) > 1939


def test_build_roi_raster_wraps_the_kernels():
    from range_view_3d_detection_amd.converters.av2.roi import build_roi_raster

    arr, (s, tx, ty) = build_roi_raster([np.asarray(p) for p in ref.POLYGONS], resolution_m=0.5, dilation_m=2.0, device=DEV)
    assert s == 2.0 and (tx, ty) == (-1.0, -2.0)  # floor(3.2 - 2), floor(4.1 - 2)
    assert arr.shape == (math.ceil((55.9 + 2.0 - 2.0) * 2) + 1, math.ceil((70.1 + 2.0 - 1.0) * 2) + 1) and arr.dtype == np.uint8
    want = ref.dilate_ref(ref.fill_ref(ref.POLYGONS, s, tx, ty, *arr.shape), 4.0)
    assert np.array_equal(arr, want) and arr.sum() > 4 * 875


def _match(scene, cfg, dt_roi, gt_roi):
    from range_view_3d_detection_amd.evaluation import match

    n_cat, n_seg = scene["n_cat"], scene["n_sweeps"] * scene["n_cat"]
    valid = scene["gt_roi"] if scene.get("gt_valid") is None else scene["gt_valid"] & scene["gt_roi"]
    out = match(_dev(scene["dts"]), _dev(scene["scores"]), _dev(scene["dt_sweep"]) * n_cat + _dev(scene["dt_cat"]), _dev(scene["gts"]),
                _dev(valid if gt_roi else scene.get("gt_valid")), _dev(scene["gt_sweep"]) * n_cat + _dev(scene["gt_cat"]), n_seg, cfg,
                dt_roi=_dev(scene["dt_roi"]) if dt_roi else None)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_matcher_applies_the_cap_before_the_roi_flag():
    s = dict(match_scene(), n_sweeps=1, n_cat=2)
    out = _match(s, s["cfg"], True, True)
    for key in ("evaluated", "tp", "matched_gt", "gt_evaluated"):
        assert np.array_equal(out[key], np.asarray(s["expect"][key])), key
    assert np.isnan(out["err"][[0, 2, 3]]).all() and np.array_equal(out["err"][1], [0.0, 0.0, 0.0])
    assert [int(out["gt_evaluated"][s["gt_cat"] == c].sum()) for c in range(2)] == s["expect"]["n_gts"]


def test_matcher_against_the_restatement_on_segments_longer_than_a_tile():
    """Segments of several hundred rows (more than one 256-row tile of the scan), a cap of 100 and of 300, random flags."""
    g = np.random.default_rng(np.random.randint(1 << 30))
    scene = _scene(g, 2, 3, max_gt=30, max_dt=200, big=(1, 2, 40))  # (that segment: 400 detections)
    scene["dt_roi"], scene["gt_roi"] = (g.random(len(scene["dts"])) < 0.6).astype(np.uint8), (g.random(len(scene["gts"])) < 0.7).astype(np.uint8)
    assert np.bincount(scene["dt_sweep"] * 3 + scene["dt_cat"]).max() > 300
    for cap in (100, 300):
        cfg = _cfg(3, max_num_dts_per_category=cap)
        out = _match(scene, cfg, True, True)
        want = ref.match_roi_ref(scene["dts"], scene["scores"], scene["dt_sweep"], scene["dt_cat"], scene["dt_roi"], scene["gts"], scene["gt_valid"],
                                 scene["gt_roi"], scene["gt_sweep"], scene["gt_cat"], 2, 3, cfg)
        for key in ("evaluated", "tp", "matched_gt", "gt_evaluated"):
            assert np.array_equal(out[key], want[key]), (cap, key)
        assert np.array_equal(np.isnan(out["err"]), np.isnan(want["err"])) and np.allclose(out["err"], want["err"], rtol=0, atol=1e-5, equal_nan=True)
        assert 50 < out["evaluated"].sum() < (scene["dt_roi"] != 0).sum()


def test_matcher_keeps_the_cap_and_the_packed_list_across_a_tile_boundary():
    """One segment of 600 detections (three tiles of the scan), more of them in range than the cap of 300, so the cap falls inside
    the second tile; flags set and clear on both sides of every tile boundary: the rank of the first scan and the slot of the second
    both carry over tiles."""
    g = np.random.default_rng(np.random.randint(1 << 30))
    scene = _scene(g, 1, 1, big=(0, 0, 40, 600))
    n, m = len(scene["dts"]), len(scene["gts"])
    assert (n, m) == (600, 40)
    scene["dt_roi"], scene["gt_roi"] = g.integers(0, 2, n).astype(np.uint8), g.integers(0, 2, m).astype(np.uint8)
    in_range = (scene["dts"][:, :3].astype(np.float64) ** 2).sum(1) <= 150.0 ** 2
    by_score = np.argsort(-scene["scores"], kind="stable")
    assert in_range.sum() > 300 and 256 < np.nonzero(np.cumsum(in_range[by_score]) == 300)[0][0] < 512
    for tile in (by_score[:256], by_score[256:512], by_score[512:]):
        assert 0 < scene["dt_roi"][tile].sum() < len(tile)
    cfg = _cfg(1, max_num_dts_per_category=300)
    out = _match(scene, cfg, True, True)
    want = ref.match_roi_ref(scene["dts"], scene["scores"], scene["dt_sweep"], scene["dt_cat"], scene["dt_roi"], scene["gts"], scene["gt_valid"],
                             scene["gt_roi"], scene["gt_sweep"], scene["gt_cat"], 1, 1, cfg)
    for key in ("evaluated", "tp", "matched_gt", "gt_evaluated"):
        assert np.array_equal(out[key], want[key]), key
    assert np.array_equal(np.isnan(out["err"]), np.isnan(want["err"])) and np.allclose(out["err"], want["err"], rtol=0, atol=1e-5, equal_nan=True)
    assert 100 < out["evaluated"].sum() < 300 and out["evaluated"][by_score[256:]].sum() > 10 and out["matched_gt"].max() >= 0
    plain = eval_ref.match_ref(scene["dts"], scene["scores"], scene["dt_sweep"], scene["dt_cat"], scene["gts"], scene["gt_valid"], scene["gt_sweep"],
                               scene["gt_cat"], 1, 1, cfg)
    assert np.array_equal(_match(scene, cfg, False, False)["evaluated"], plain["evaluated"]) and plain["evaluated"].sum() == 300


def _small_scene(g):
    """The existing evaluation test's scene scaled down: 4 sweeps x 5 categories, 200 detections with tied scores, rows by sweep."""
    scene = _scene(g, 4, 5, max_gt=12, max_dt=60)
    pick = np.sort(g.permutation(len(scene["dts"]))[:200])
    for k in ("dts", "scores", "dt_sweep", "dt_cat"):
        scene[k] = scene[k][pick]
    assert len(np.unique(scene["scores"])) < 150
    return scene


def _annotations(scene):
    ann = np.zeros((len(scene["gts"]), 13))
    ann[:, :10], ann[:, 11], ann[:, 12] = scene["gts"], scene["gt_cat"], scene["gt_sweep"]
    return ann


def test_an_all_covering_roi_changes_nothing():
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.evaluation import DetectionEvaluator

    g = np.random.default_rng(np.random.randint(1 << 30))
    scene = _small_scene(g)
    names = [f"C{i}" for i in range(5)]
    args = (_dev(scene["dts"]), _dev(scene["scores"]), _dev(scene["dt_cat"], torch.float32), _dev(scene["dt_sweep"], torch.float32), _dev(_annotations(scene)))
    npts = _dev(scene["gt_valid"])
    plain = DetectionEvaluator(_cfg(5), names, max_sweeps=4)
    for _ in range(2):
        plain.update(*args, num_interior_pts=npts)
    # every vertex lies within +-200 m: a raster of ones from -250 to 250 m covers them under the identity pose
    atlas = _atlas([(np.ones((500, 500), np.uint8), (1.0, 250.0, 250.0))])
    roi = (_dev(np.zeros(4, np.int32)), _dev(np.tile(np.eye(4)[:3], (4, 1, 1))))
    filtered = DetectionEvaluator(_cfg(5, eval_only_roi_instances=True), names, max_sweeps=4, atlas=atlas)
    filtered.update(*args, num_interior_pts=npts, roi=roi)  # (first call: library load, lookup tables)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        filtered.update(*args, num_interior_pts=npts, roi=roi)  # nothing is read back with the filter on either
    finally:
        torch.cuda.set_sync_debug_mode("default")
    table = plain.compute()
    assert filtered.compute().equals(table) and 0 < table.column("AP")[-1].as_py() < 1

    # rv_eval_match_roi without flags is rv_eval_match, array for array
    n_cat, n_seg, n, m = 5, 20, len(scene["dts"]), len(scene["gts"])
    from range_view_3d_detection_amd.evaluation.rows import order_rows

    dts, gts, valid = _dev(scene["dts"]), _dev(scene["gts"]), _dev(scene["gt_valid"])
    dt_order, dt_off, gt_order, gt_off = order_rows(_dev(scene["dt_sweep"]) * n_cat + _dev(scene["dt_cat"]), _dev(scene["scores"]),
                                                    _dev(scene["gt_sweep"]) * n_cat + _dev(scene["gt_cat"]), n_seg)
    thr = (ctypes.c_double * 4)(0.5, 1.0, 2.0, 4.0)
    results = []
    for name in ("rv_eval_match", "rv_eval_match_roi"):
        out = [torch.full((n,), 7, dtype=torch.uint8, device=DEV), torch.full((n, 4), 7, dtype=torch.uint8, device=DEV),
               torch.full((n, 3), 7.0, dtype=torch.float32, device=DEV), torch.full((n,), 7, dtype=torch.int32, device=DEV),
               torch.full((m,), 7, dtype=torch.uint8, device=DEV)]
        flags = (ctypes.c_void_p(0),) if name == "rv_eval_match_roi" else ()
        L.call(name, L.ptr(dts), L.ptr(dt_order), L.ptr(dt_off), n, L.ptr(gts), L.ptr(valid), L.ptr(gt_order), L.ptr(gt_off), m,
               n_seg, thr, 4, 2.0, 150.0, 100, *flags, *[L.ptr(t) for t in out], L.stream_ptr())
        results.append([t.cpu().numpy() for t in out])
    for a, b in zip(*results):
        assert np.array_equal(a, b, equal_nan=True)
    assert results[0][0].sum() > 50 and results[0][3].max() >= 0


def test_update_with_a_half_plane_roi_equals_the_offline_form():
    """``update(..., roi=)`` + ``compute`` against ``evaluate(dts, gts, cfg, atlas=, poses=)`` on the same rows as Arrow tables, and both
    against the restatement's flags and counts.  Two logs: x >= 0 of the city frame is ROI in one, y >= 0 in the other; every sweep has
    its own pose."""
    import pyarrow as pa

    from range_view_3d_detection_amd._lib import RvError
    from range_view_3d_detection_amd.evaluation import DetectionEvaluator, evaluate
    from range_view_3d_detection_amd.math.ops.coding import DETECTION_COLUMNS

    g = np.random.default_rng(np.random.randint(1 << 30))
    scene = _small_scene(g)
    half_x, half_y = np.zeros((800, 800), np.uint8), np.zeros((800, 800), np.uint8)
    half_x[:, 400:], half_y[400:, :] = 1, 1
    layers, log_names = [(half_x, (1.0, 400.0, 400.0)), (half_y, (1.0, 400.0, 400.0))], ["logX", "logY"]
    layer_index = np.array([0, 0, 1, 1])
    poses = np.stack([_random_pose(g) for _ in range(4)])
    poses[:, :, 3] = g.uniform(-60, 60, (4, 3))  # the boxes (within 200 m of the ego vehicle) straddle the half-plane's edge
    dt_roi, _ = ref.boxes_ref(scene["dts"], scene["dt_sweep"], layer_index, poses, layers)
    gt_roi, _ = ref.boxes_ref(scene["gts"], scene["gt_sweep"], layer_index, poses, layers)
    assert 0.2 < dt_roi.mean() < 0.8 and 0.2 < gt_roi.mean() < 0.8
    cfg, names = _cfg(5, eval_only_roi_instances=True), [f"C{i}" for i in range(5)]
    want = ref.match_roi_ref(scene["dts"], scene["scores"], scene["dt_sweep"], scene["dt_cat"], dt_roi, scene["gts"], scene["gt_valid"], gt_roi,
                             scene["gt_sweep"], scene["gt_cat"], 4, 5, cfg)
    want_n_dts = [int(np.sum((scene["dt_cat"] == c) & (want["evaluated"] != 0))) for c in range(5)]
    want_n_gts = [int(np.sum((scene["gt_cat"] == c) & (want["gt_evaluated"] != 0))) for c in range(5)]

    atlas = _atlas(layers, log_names)
    ev = DetectionEvaluator(cfg, names, max_sweeps=64, atlas=atlas)
    ev.update(_dev(scene["dts"]), _dev(scene["scores"]), _dev(scene["dt_cat"], torch.float32), _dev(scene["dt_sweep"], torch.float32),
              _dev(_annotations(scene)), num_interior_pts=_dev(scene["gt_valid"]), roi=(_dev(layer_index), _dev(poses)))
    online = ev.compute()
    assert online.column("n_dts").to_pylist()[:-1] == want_n_dts and online.column("n_gts").to_pylist()[:-1] == want_n_gts

    log_of, ts_of = [log_names[layer_index[s]] for s in range(4)], [1000 + s for s in range(4)]
    frame = lambda rows, sweep, cat, extra: pa.table({**{c: pa.array(rows[:, j]) for j, c in enumerate(DETECTION_COLUMNS)},  # noqa: E731
                                                      "category": [names[c] for c in cat], "log_id": [log_of[s] for s in sweep],
                                                      "timestamp_ns": [ts_of[s] for s in sweep], **extra})
    dts = frame(scene["dts"], scene["dt_sweep"], scene["dt_cat"], {"score": pa.array(scene["scores"])})
    gts = frame(scene["gts"], scene["gt_sweep"], scene["gt_cat"], {"num_interior_pts": pa.array(scene["gt_valid"].astype(np.int64))})
    pose_of = {(log_of[s], ts_of[s]): poses[s] for s in range(4)}
    dts_out, gts_out, offline = evaluate(dts, gts, cfg, device=DEV, atlas=atlas.to("cpu"), poses=pose_of)
    assert offline.equals(online)
    assert np.array_equal(np.asarray(dts_out.column("is_within_roi").to_pylist()), dt_roi != 0)
    assert np.array_equal(np.asarray(gts_out.column("is_within_roi").to_pylist()), gt_roi != 0)
    assert np.array_equal(np.asarray(dts_out.column("is_evaluated").to_pylist()), want["evaluated"] != 0)
    assert np.array_equal(np.asarray(gts_out.column("is_evaluated").to_pylist()), want["gt_evaluated"] != 0)
    assert np.array_equal(np.asarray(dts_out.column("tp_2.0").to_pylist()), want["tp"][:, 2] != 0)
    # fewer boxes count than without the filter, and the table says so
    plain = eval_ref.match_ref(scene["dts"], scene["scores"], scene["dt_sweep"], scene["dt_cat"], scene["gts"], scene["gt_valid"], scene["gt_sweep"],
                               scene["gt_cat"], 4, 5, cfg)
    assert sum(want_n_gts) < plain["gt_evaluated"].sum() and sum(want_n_dts) < plain["evaluated"].sum()
    del pose_of[(log_of[2], ts_of[2])]
    with pytest.raises(RvError, match=r"no city_SE3_ego for sweep .*logY.*1002"):
        evaluate(dts, gts, cfg, device=DEV, atlas=atlas, poses=pose_of)
