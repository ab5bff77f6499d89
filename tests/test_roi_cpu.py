"""AV2 ROI, the part that needs no GPU: the NumPy restatement of the declared semantics (``tests/roi_ref.py``) against the hand-worked
cases of ``tests/golden/roi_cases.json``, the fill and the dilation against independent implementations (matplotlib, scipy), the
exports of both builds, the host-side checks of the atlas, the configuration factory and the ``RvError`` paths of the evaluator."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import roi_ref as ref
from test_evaluation_cpu import _cfg

CASES = ref.load_cases()
ROI_SYMBOLS = ("rv_roi_atlas_check", "rv_roi_points", "rv_roi_boxes", "rv_roi_rasterize", "rv_roi_rasterize_workspace_bytes", "rv_eval_match_roi")


def match_scene(cases=CASES):
    """The cap-rule scene of the golden file as the arrays ``match_roi_ref`` / ``match`` take (one sweep, two categories)."""
    import eval_ref

    m = cases["match"]
    n, k = len(m["dts"]), len(m["gts"])
    return {"dts": eval_ref.rows_from_yaw(m["dts"]), "scores": np.asarray(m["scores"], np.float32), "dt_sweep": np.zeros(n, np.int64),
            "dt_cat": np.asarray(m["dt_cat"], np.int64), "dt_roi": np.asarray(m["dt_roi"], np.uint8), "gts": eval_ref.rows_from_yaw(m["gts"]),
            "gt_sweep": np.zeros(k, np.int64), "gt_cat": np.asarray(m["gt_cat"], np.int64), "gt_roi": np.asarray(m["gt_roi"], np.uint8),
            "cfg": _cfg(2, max_num_dts_per_category=m["max_num_dts_per_category"]), "expect": m["expect"]}


def test_restatement_equals_the_hand_worked_points():
    p = CASES["points"]
    got, stray = ref.lookup_ref(p["xyz"], p["sweep"], CASES["layer_index"], CASES["poses"], CASES["layers"])
    assert stray == 0
    wrong = [p["why"][i] for i in np.nonzero(got != p["expect"])[0]]
    assert not wrong, wrong
    # the same points rounded to fp32 on the way in (the boundary cases are fp32 numbers; the others sit well inside their cells)
    got32, _ = ref.lookup_ref(p["xyz"].astype(np.float32), p["sweep"], CASES["layer_index"], CASES["poses"], CASES["layers"])
    assert np.array_equal(got32, got)


def test_restatement_equals_the_hand_worked_boxes():
    b = CASES["boxes"]
    got, stray = ref.boxes_ref(b["rows"], b["sweep"], CASES["layer_index"], CASES["poses"], CASES["layers"])
    assert stray == 0
    wrong = [b["why"][i] for i in np.nonzero(got != b["expect"])[0]]
    assert not wrong, wrong
    # the tilted box reaches the strip with exactly one vertex
    v = ref.box_vertices_ref(b["rows"][2:3])[0]
    assert np.sum((v[:, 0] >= 4) & (v[:, 0] < 5)) == 1 and np.allclose(v[:, 0].max(), 4.32, atol=1e-6)


def test_a_row_outside_every_sweep_is_stray():
    layers, li, poses = CASES["layers"], CASES["layer_index"], CASES["poses"]
    got, stray = ref.lookup_ref([[-2.0, -3.0, 0.0]] * 3, [0, -1, len(li)], li, poses, layers)
    assert got.tolist() == [1, 0, 0] and stray == 2
    assert ref.sweep_of_rows([2, 5, 5, 6], 8).tolist() == [-1, -1, 0, 0, 0, 2, -1, -1]  # an empty sweep is passed over


def test_the_cases_cover_what_the_declaration_singles_out():
    p, b = CASES["points"], CASES["boxes"]
    why = " | ".join(p["why"] + b["why"])
    for needle in ("exactly on a cell boundary", "a = -0.5", "a = -1.0", "u == width", "v == height", "NaN", "layer index -1", "90 degree turn",
                   "general pose", "centre outside", "across the strip", "tilted box"):
        assert needle in why, needle
    s = sorted(l[1][0] for l in CASES["layers"])
    assert s[0] == 1.0 and s[-1] == 1 / 0.3 and len({l[1][1:] for l in CASES["layers"]}) == 3
    assert np.isnan(p["xyz"]).any() and np.isinf(p["xyz"]).any()
    # the boundary point is dyadic: no rounding anywhere on its way to the cell
    x = p["xyz"][1, 0]
    assert x == -(1 + 2.0 ** -20) and np.float32(x) == x


def test_fill_against_matplotlib_and_dilation_against_scipy():
    """The declared pixel-centre even-odd fill and the `<=` dilation against two libraries, on the issue's polygons: equality on
    every pixel."""
    from matplotlib.path import Path
    from scipy.ndimage import distance_transform_edt

    g = ref.POLYGON_RASTER
    drivable = ref.fill_ref(ref.POLYGONS, g["s"], g["tx"], g["ty"], g["height"], g["width"])
    uu, vv = np.meshgrid(np.arange(g["width"]) + 0.5, np.arange(g["height"]) + 0.5)
    centres = np.stack([uu.ravel(), vv.ravel()], 1)
    want = np.zeros(g["height"] * g["width"], bool)
    for poly in ref.POLYGONS:
        mapped = (np.asarray(poly) + [g["tx"], g["ty"]]) * g["s"]
        want |= Path(mapped).contains_points(centres)
    assert np.array_equal(drivable.astype(bool), want.reshape(g["height"], g["width"]))
    assert int(drivable.sum()) == 875
    for r in (5.0, 16.5):
        roi = ref.dilate_ref(drivable, r)
        assert np.array_equal(roi.astype(bool), distance_transform_edt(drivable == 0) <= r), r
    assert int(ref.dilate_ref(drivable, 5.0).sum()) == 1939
    assert np.array_equal(ref.dilate_ref(drivable, 0.0), drivable)


def test_matcher_restatement_applies_the_cap_before_the_roi_flag():
    s = match_scene()
    out = ref.match_roi_ref(s["dts"], s["scores"], s["dt_sweep"], s["dt_cat"], s["dt_roi"], s["gts"], None, s["gt_roi"], s["gt_sweep"], s["gt_cat"],
                            1, 2, s["cfg"])
    for key in ("evaluated", "tp", "matched_gt", "gt_evaluated"):
        assert np.array_equal(out[key], np.asarray(s["expect"][key])), key
    assert np.isnan(out["err"][[0, 2, 3]]).all() and np.array_equal(out["err"][1], [0.0, 0.0, 0.0])
    n_gts = [int(np.sum((s["gt_cat"] == c) & (out["gt_evaluated"] != 0))) for c in range(2)]
    assert n_gts == s["expect"]["n_gts"]
    # all flags set: the plain matcher
    import eval_ref

    ones = ref.match_roi_ref(s["dts"], s["scores"], s["dt_sweep"], s["dt_cat"], np.ones(4, np.uint8), s["gts"], None, np.ones(2, np.uint8),
                             s["gt_sweep"], s["gt_cat"], 1, 2, s["cfg"])
    plain = eval_ref.match_ref(s["dts"], s["scores"], s["dt_sweep"], s["dt_cat"], s["gts"], None, s["gt_sweep"], s["gt_cat"], 1, 2, s["cfg"])
    for key in plain:
        assert np.array_equal(ones[key], plain[key], equal_nan=True), key


@pytest.mark.parametrize("tag", ["bf16", "f16"])
def test_both_builds_export_the_roi_entry_points(tag):
    from range_view_3d_detection_amd import _lib

    handle = _lib.load(tag)
    assert set(ROI_SYMBOLS) <= set(_lib.declared_symbols())
    assert all(hasattr(handle, s) for s in ROI_SYMBOLS)
    assert ctypes.sizeof(_lib.RoiLayer) == 40
    # 32 bytes per polygon + 4 bytes per pixel, each part rounded up to 256 bytes
    assert handle.rv_roi_rasterize_workspace_bytes(2, 80, 96) == 256 + 80 * 96 * 4
    assert handle.rv_roi_rasterize_workspace_bytes(2, 0, 96) == 0


def test_atlas_is_built_and_checked_on_the_host():
    from range_view_3d_detection_amd._lib import RvError
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.converters.av2.roi import RoiAtlas

    arrays, sims = [l[0] for l in CASES["layers"]], [l[1] for l in CASES["layers"]]
    atlas = RoiAtlas.from_rasters(CASES["layer_names"], arrays, sims)
    assert atlas.n_layers == 3 and atlas.raster.numel() == 20 + 9 + 64 and atlas.layers.numel() == 3 * 40 and atlas.device.type == "cpu"
    assert atlas.records["offset"].tolist() == [0, 20, 29] and atlas.records["width"].tolist() == [5, 3, 8]
    assert [atlas.layer_of(n) for n in CASES["layer_names"]] == [0, 1, 2]
    arr, sim = atlas.layer(1)
    assert np.array_equal(arr, arrays[1]) and sim == sims[1]
    with pytest.raises(RvError, match="no raster for log"):
        atlas.layer_of("nowhere")
    with pytest.raises(RvError, match="twice"):
        RoiAtlas.from_rasters(["a", "a"], arrays[:2], sims[:2])
    with pytest.raises(RvError, match="s = "):
        RoiAtlas.from_rasters(["a"], arrays[:1], [(0.0, 1.0, 1.0)])
    # a table whose layer reaches beyond the buffer is refused before any kernel could read through it
    table = (L.RoiLayer * 2)(L.RoiLayer(0, 4, 5, 1.0, 0.0, 0.0), L.RoiLayer(20, 3, 3, 1.0, 0.0, 0.0))
    L.call("rv_roi_atlas_check", table, 2, 29)
    with pytest.raises(RvError, match="reaches beyond"):
        L.call("rv_roi_atlas_check", table, 2, 28)
    table[1].offset = -1
    with pytest.raises(RvError, match="reaches beyond"):
        L.call("rv_roi_atlas_check", table, 2, 29)


def test_argument_checks_need_no_device():
    from range_view_3d_detection_amd import _lib as L

    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)
    with pytest.raises(L.RvError, match="sweeps"):
        L.call("rv_roi_points", null, 0, 0, one, 0, one, one, null, 0, null, 0, null, one, null)
    with pytest.raises(L.RvError, match="null sweep table"):
        L.call("rv_roi_boxes", null, null, 0, 1, null, one, null, 0, null, 0, null, one, null)
    with pytest.raises(L.RvError, match="dilation radius"):
        L.call("rv_roi_rasterize", one, one, 0, 0, 1.0, 0.0, 0.0, 4, 4, -1.0, one, one, one, null)
    with pytest.raises(L.RvError, match="raster of"):
        L.call("rv_roi_rasterize", one, one, 0, 0, 1.0, 0.0, 0.0, 65536, 65536, 1.0, one, one, one,
               null)


def test_factory_keyword():
    from range_view_3d_detection_amd._lib import RvError
    from range_view_3d_detection_amd.evaluation import DetectionCfg, detection_cfg_factory

    assert DetectionCfg().eval_only_roi_instances is False
    assert detection_cfg_factory("av2", ["A"]) == detection_cfg_factory("av2", ["A"], None) == detection_cfg_factory("av2", ["A"], eval_only_roi_instances=False)
    assert detection_cfg_factory("av2", ["A"]).eval_only_roi_instances is False
    cfg = detection_cfg_factory("AV2", ["B", "A"], eval_only_roi_instances=True)
    assert cfg.eval_only_roi_instances is True and cfg.max_range_m == 150.0 and cfg.categories == ("A", "B")
    for name in ("waymo", "nuscenes", "nuscenes-mini"):
        assert detection_cfg_factory(name, ["A"], eval_only_roi_instances=False).eval_only_roi_instances is False
        with pytest.raises(RvError, match="eval_only_roi_instances"):
            detection_cfg_factory(name, ["A"], eval_only_roi_instances=True)


def test_the_filter_and_its_inputs_go_together():
    from range_view_3d_detection_amd._lib import RvError
    from range_view_3d_detection_amd.converters.av2.roi import RoiAtlas
    from range_view_3d_detection_amd.evaluation import DetectionEvaluator, evaluate

    atlas = RoiAtlas.from_rasters(["a"], [np.ones((2, 2), np.uint8)], [(1.0, 0.0, 0.0)])
    on, off = _cfg(2, eval_only_roi_instances=True), _cfg(2)
    rows = (torch.zeros(3, 10), torch.zeros(3), torch.zeros(3), torch.zeros(3), torch.zeros(0, 13, dtype=torch.float64))
    roi = (torch.zeros(1, dtype=torch.int32), torch.eye(4, dtype=torch.float64)[None, :3])
    with pytest.raises(RvError, match="no atlas was given"):  # the flag without the rasters
        DetectionEvaluator(on, ["C0", "C1"])
    with pytest.raises(RvError, match="no roi was given"):  # the flag without the step's sweep table
        DetectionEvaluator(on, ["C0", "C1"], atlas=atlas).update(*rows)
    with pytest.raises(RvError, match="roi given while"):  # the sweep table without the flag
        DetectionEvaluator(off, ["C0", "C1"]).update(*rows, roi=roi)
    with pytest.raises(RvError, match="atlas given while"):
        DetectionEvaluator(off, ["C0", "C1"], atlas=atlas)
    with pytest.raises(RvError, match="no atlas / poses"):
        evaluate(None, None, on, device="cpu", atlas=atlas)
    with pytest.raises(RvError, match="atlas / poses given while"):
        evaluate(None, None, off, device="cpu", poses={})
    with pytest.raises(RvError, match="no CPU fallback"):  # with everything in place the rows still have to be on a device
        DetectionEvaluator(on, ["C0", "C1"], atlas=atlas).update(*rows, roi=roi)
