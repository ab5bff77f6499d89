"""The debug panels on the device (``csrc/render.hip``, ``rendering/tensorboard.py``, ``compat/mmcv_ops.py``) against the NumPy
restatement ``tests/render_ref.py`` -- bit for bit wherever the declared arithmetic is IEEE operations only.  Tiny shapes: H 4 or 8 with
W 40, 64 and 37 against a 40-pixel view (``max_side = 3.0``: both padding branches and an odd difference)."""

from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import render_ref as R  # noqa: E402
from test_render_cpu import fixture_panels  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ULP4 = 4 * 2.0 ** -23  # 4 fp32 ulps of 1 (4.8e-7): one add, one divide and expf's stated 1 to 2 ulps


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _tb():
    from range_view_3d_detection_amd.rendering import tensorboard as tb

    return tb


def _tables():
    tb = _tb()
    return {k: getattr(tb, k).numpy() for k in ("GREYS", "TURBO_R", "VIRIDIS")}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- planes and the colormap pass ------------------------------------------------------------------------------------------------
def _device_plane(src, op):
    tb = _tb()
    src = _dev(src, torch.float32)
    plane = torch.empty(src.shape[-2:], dtype=torch.float32, device=DEV)
    minmax = torch.zeros(2, dtype=torch.int32, device=DEV)
    tb._plane(src, op, plane, minmax)
    return plane, minmax


@pytest.mark.parametrize("H,W", [(4, 40), (8, 64), (4, 37)])
@pytest.mark.parametrize("case", ["random", "constant", "all_masked", "single_max"])
def test_planes_and_colormap(H, W, case):
    tb, tables = _tb(), _tables()
    g = np.random.default_rng(H * 1000 + W)
    if case == "constant":
        cart, logits, aux = np.full((3, H, W), 1.5, np.float32), np.full((3, H, W), -0.75, np.float32), np.full((1, H, W), -2.0, np.float32)
    elif case == "single_max":
        cart, logits, aux = np.zeros((3, H, W), np.float32), np.full((3, H, W), -8.0, np.float32), np.zeros((1, H, W), np.float32)
        cart[:, H - 1, W - 1], logits[1, 2, 5], aux[0, 0, 0] = (3.0, -4.0, 12.0), 6.0, -9.0
    else:
        cart = (g.standard_normal((3, H, W)) * 30.0).astype(np.float32)
        logits, aux = (g.standard_normal((3, H, W)) * 4 - 2).astype(np.float32), g.standard_normal((1, H, W)).astype(np.float32)
    mask = np.zeros((H, W), bool) if case == "all_masked" else g.random((H, W)) > 0.25
    side = 40
    W_total, col0 = max(W, side), (side - W) // 2 if W < side else 0
    for src, op, table in ((cart, tb.PLANE_NORM, "TURBO_R"), (logits, tb.PLANE_LIKELIHOOD, "VIRIDIS"), (aux, tb.PLANE_ABS, "VIRIDIS"),
                           (aux, tb.PLANE_IDENTITY, "GREYS")):
        plane, minmax = _device_plane(src, op)
        p = plane.cpu().numpy()
        if op == tb.PLANE_NORM:
            assert np.array_equal(_bits(p), _bits(R.plane_norm(cart)))
        elif op == tb.PLANE_ABS:
            assert np.array_equal(_bits(p), _bits(R.plane_abs(aux[0])))
        elif op == tb.PLANE_IDENTITY:
            assert np.array_equal(_bits(p), _bits(aux[0]))
        else:
            err = float(np.abs(p.astype(np.float64) - R.plane_likelihood64(logits)).max())
            print(f"likelihood plane {H}x{W} {case}: max |device - float64| = {err:.3e} (bound {ULP4:.3e})")
            assert err <= ULP4
        # the device's plane through the device colormap pass, against the restatement fed the DEVICE's plane
        image = torch.zeros((3, H + 3, W_total), dtype=torch.uint8, device=DEV)
        tb._colormap(plane, _dev(mask, torch.uint8), minmax, tb._lut(table, DEV), image, 2, col0)
        want = np.zeros((3, H + 3, W_total), np.uint8)
        want[:, 2:2 + H, col0:col0 + W] = R.normalize_apply_colormap(p, tables[table], mask)
        assert np.array_equal(image.cpu().numpy(), want), (op, table)
        if case == "constant":
            assert (R.colormap_index(p) == 0).all()
        if case == "all_masked":
            assert not image.any()
    # the public function with the reference's signature: a (3,256) tensor as the colormap, no mask
    out = tb.normalize_apply_colormap(_dev(aux).view(1, 1, H, W), tb.TURBO_R)
    assert np.array_equal(out.cpu().numpy(), R.normalize_apply_colormap(aux[0], tables["TURBO_R"]))


# ---- bird's-eye view: points -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_side,mpp", [(3.0, 0.15), (4.0, 0.25), (75.0, 0.15)])
def test_point_splat(max_side, mpp):
    tb = _tb()
    g = np.random.default_rng(3)
    n = 3000
    xyz = ((g.random((n, 3)) - 0.5) * 2.4 * max_side).astype(np.float32)
    xyz[:40] = 0.0  # norm 0
    ulp = np.float32(max_side) - np.nextafter(np.float32(max_side), np.float32(0))
    specials = [(-max_side, 0.5), (max_side, 0.5), (0.5, -max_side), (0.5, max_side),  # u == 0 and u == size (or the last pixel)
                (-max_side + ulp, 0.25), (0.25, -max_side + ulp),  # a tiny u: size - u rounds to size, row / column `side`
                (max_side - ulp, -0.25), (np.nan, 0.0), (0.0, np.inf)]
    xyz[40:40 + len(specials), :2] = np.asarray(specials, np.float32)
    xyz[40:40 + len(specials), 2] = 1.0
    side = R.bev_side(max_side, mpp)
    want = R.bev_points(xyz.T, max_side, mpp)
    got = tb.build_bev(_dev(xyz), max_side, mpp)
    assert tuple(got.shape) == (side, side, 3)
    assert np.array_equal(got.permute(2, 0, 1).cpu().numpy(), want)
    assert 100 < int((want[0] > 0).sum()) < n
    (kx, r), (ky, c) = R.world_to_image(xyz[:, 0], max_side, mpp), R.world_to_image(xyz[:, 1], max_side, mpp)
    keep = kx & ky
    assert np.array_equal(tb.world_to_image(_dev(xyz), max_side, mpp).cpu().numpy(), np.stack([r[keep], c[keep], xyz[keep, 2]], 1))
    if mpp == 0.25:  # exact arithmetic: u == 0 and u == 32 are outside; the tiny u is kept, lands on row 32 = side and is dropped
        kept, r = R.world_to_image(np.float32(-max_side + ulp), max_side, mpp)
        assert kept and r == side
        assert not R.world_to_image(np.float32(max_side), max_side, mpp)[0] and not R.world_to_image(np.float32(-max_side), max_side, mpp)[0]


# ---- bird's-eye view: boxes --------------------------------------------------------------------------------------------------------
def _device_boxes(bev, boxes, scores, channels, max_side, mpp):
    tb = _tb()
    image = _dev(bev).clone()
    side = image.shape[1]
    tb._bev_boxes(_dev(np.asarray(boxes, np.float32).reshape(-1, 7)), None if scores is None else _dev(scores, torch.float32),
                  _dev(np.asarray(channels, np.uint8)), max_side, mpp, side, image, 0, 0)
    return image.cpu().numpy()


def test_boxes_on_the_hand_worked_cases():
    with open(os.path.join(HERE, "golden", "render_cases.json")) as f:
        cases = json.load(f)
    v = cases["view"]
    ms, mpp, side = v["max_side"], v["meter_per_px"], v["side"]
    for c in cases["boxes"]:
        bev = np.zeros((3, side, side), np.uint8)
        bev[:, 15, 18] = 255
        got = _device_boxes(bev, c["boxes"], c["scores"], c["channels"], ms, mpp)
        assert np.array_equal(got, R.draw_boxes(bev, c["boxes"], c["scores"], c["channels"], ms, mpp)), c["name"]
        for r, cc, rgb in c["probes"]:
            assert got[:, r, cc].tolist() == rgb, (c["name"], r, cc)


def test_boxes_seeded_and_repeatable():
    g = np.random.default_rng(17)
    n, ms, mpp = 200, 10.0, 0.2
    side = R.bev_side(ms, mpp)
    boxes = np.zeros((n, 7), np.float32)
    boxes[:, :2] = (g.random((n, 2)) - 0.5) * 2.3 * ms  # some partly, some wholly outside
    boxes[:, 3:6] = np.asarray([4.5, 2.0, 1.7]) * (0.3 + g.random((n, 3)) * 1.2)
    boxes[:, 6] = (g.random(n) * 2 - 1) * math.pi
    boxes[5, 3:5] = 0.0  # a point: zero-length segments
    boxes[6] = boxes[7]  # an exact duplicate under a different colour
    scores = np.round(g.random(n) * 64) / 64
    scores[:3] = (0.0, 1.0, 1.5)
    channels = g.choice([R.RED, R.GREEN, R.BLUE, R.RED | R.GREEN | R.BLUE], n).astype(np.uint8)
    channels[6], channels[7] = R.RED, R.GREEN
    bev = (g.random((1, side, side)) > 0.9).astype(np.uint8).repeat(3, 0) * 255
    want = R.draw_boxes(bev, boxes, scores, channels, ms, mpp)
    got = _device_boxes(bev, boxes, scores, channels, ms, mpp)
    assert np.array_equal(got, want)
    assert int((want != bev).any(0).sum()) > 2000
    for _ in range(3):
        assert np.array_equal(_device_boxes(bev, boxes, scores, channels, ms, mpp), got)
    # scores = NULL draws at 255
    assert np.array_equal(_device_boxes(bev, boxes[:20], None, channels[:20], ms, mpp), R.draw_boxes(bev, boxes[:20], None, channels[:20], ms, mpp))


# ---- rv_boxes_iou3d ----------------------------------------------------------------------------------------------------------------
def _random_boxes(g, n, spread):
    b = np.zeros((n, 7))
    b[:, :2] = (g.random((n, 2)) - 0.5) * 2 * spread
    b[:, 2] = g.standard_normal(n) * 0.5
    b[:, 3:6] = np.asarray([4.5, 2.0, 1.7]) * (0.5 + g.random((n, 3)))
    b[:, 6] = (g.random(n) * 2 - 1) * math.pi
    return b.astype(np.float32)


def test_iou3d_equals_the_waymo_column_and_the_float64_clip():
    from range_view_3d_detection_amd.compat.mmcv_ops import boxes_iou3d
    from range_view_3d_detection_amd.evaluation import waymo as W

    g = np.random.default_rng(23)
    n, m = 300, 200
    b = _random_boxes(g, m, 20.0)  # within 30 m
    a = _random_boxes(g, n, 20.0)
    a[:m] = b + (g.standard_normal((m, 7)) * (0.4, 0.4, 0.2, 0.2, 0.1, 0.1, 0.1)).astype(np.float32)  # near-duplicates: real overlaps
    a[7], a[8, 3], a[9, 5] = b[7], 0.0, 0.0  # identical; no area; no volume
    got = boxes_iou3d(_dev(a), _dev(b))
    assert tuple(got.shape) == (n, m) and got.dtype == torch.float32
    ws = W.pairwise_iou(_dev(a), _dev(np.arange(n)), _dev(np.asarray([0, n])), _dev(b), _dev(np.arange(m)), _dev(np.asarray([0, m])), 1)
    _, table = W._workspace_views(ws, 1)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(table[:n * m, 1].reshape(n, m).cpu().numpy()))
    want = R.boxes_iou3d64(a, b)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"rv_boxes_iou3d against the float64 clip: max error {err:.3e}")
    assert err <= 1e-5
    assert (want > 0.3).sum() > 100 and abs(float(got[7, 7]) - 1.0) <= 1e-6 and float(got[8].max()) == 0.0 and float(got[9].max()) == 0.0


def test_iou3d_thresholds_colour_green_and_red_and_long_lists():
    """7 x 1 in 10 x 1 with equal heights: fp32 7 / 10 is the fp32 0.7 the colour rule compares with (green); 11 x 1 in 16 x 1: 0.6875
    (red) -- the geometry of tests/golden/waymo_eval_cases.json.  1500 x 3 rows: no limit on the row counts."""
    from range_view_3d_detection_amd.compat.mmcv_ops import boxes_iou3d

    tb = _tb()
    gts = np.asarray([[0, 0, 0, 10, 1, 2, 0], [0, 6, 0, 16, 1, 2, 0]], np.float32)
    dts = np.asarray([[0, 0, 0, 7, 1, 2, 0], [0, 6, 0, 11, 1, 2, 0]], np.float32)
    iou = boxes_iou3d(_dev(dts), _dev(gts)).cpu().numpy()
    assert iou[0, 0] == np.float32(0.7) and iou[1, 1] == np.float32(0.6875) and iou[0, 1] == 0 and iou[1, 0] == 0
    assert R.detection_channels(iou.max(1)).tolist() == [R.GREEN, R.RED]
    # through draw_detections: the colours on the view
    cart = torch.zeros((1, 3, 4, 40), device=DEV)
    outputs = {"head": {1: {"cart": cart, "mask": torch.ones((1, 1, 4, 40), dtype=torch.bool, device=DEV), 0: {"logits": torch.zeros((1, 2, 4, 40), device=DEV)}}}}
    rows = lambda b: np.concatenate([b[:, :6], np.cos(b[:, 6:] / 2), np.zeros((len(b), 2), np.float32), np.sin(b[:, 6:] / 2)], 1)  # noqa: E731
    ann = torch.from_numpy(np.concatenate([rows(gts), np.zeros((2, 3), np.float32)], 1))
    frame = {**{c: rows(dts)[:, j] for j, c in enumerate(tb.COLS)}, "score": np.asarray([1.0, 1.0], np.float32), "batch_index": np.asarray([0, 0])}
    rec = {}
    img = tb._draw(frame, {"annotations": ann}, outputs, 500, 10.0, 0.25, record=rec).cpu().numpy()
    assert rec["iou"].cpu().numpy().max(1).tolist() == [np.float32(0.7), np.float32(0.6875)]
    bev = img[:, 12:, :]
    px = lambda x, y: (int(math.floor(80 - (x + 10) / 0.25)), int(math.floor(80 - (y + 10) / 0.25)))  # noqa: E731
    at = lambda x, y: bev[(slice(None),) + px(x, y)].tolist()  # noqa: E731
    assert at(3.5, 0.0) == [0, 255, 0]   # the front of the 7 x 1 detection: green
    assert at(5.5, 6.0) == [255, 0, 0]   # the front of the 11 x 1 detection: red
    assert at(5.0, 0.0) == [0, 0, 255]   # the front of the 10 x 1 annotation: blue
    big = _random_boxes(np.random.default_rng(1), 1500, 30.0)
    out = boxes_iou3d(_dev(big), _dev(big[:3]))
    assert tuple(out.shape) == (1500, 3) and np.allclose(out[:3].diagonal().cpu().numpy(), 1.0, atol=1e-6)


# ---- draw_detections ---------------------------------------------------------------------------------------------------------------
def _restate(rec, max_side, mpp, cart0):
    """The image from the device's planes and IoU by the restatement."""
    tables = _tables()
    rgb = [R.normalize_apply_colormap(p.cpu().numpy(), tables[t], m.reshape(p.shape).cpu().numpy())
           for p, t, m in zip(rec["planes"], rec["tables"], rec["masks"])]
    bev = R.bev_points(cart0, max_side, mpp)
    ann, det = R_boxes(rec["annotations"]), R_boxes(rec["detections"])
    if len(ann):
        boxes, scores, chans = ann, np.ones(len(ann), np.float32), np.full(len(ann), R.BLUE, np.uint8)
        if rec["iou"] is not None:
            boxes, scores = np.concatenate([ann, det]), np.concatenate([scores, rec["scores"]])
            chans = np.concatenate([chans, R.detection_channels(rec["iou"].cpu().numpy().max(1))])
        bev = R.draw_boxes(bev, boxes, scores, chans, max_side, mpp)
    return R.stack(rgb, rec["kinds"], bev)


def R_boxes(rows):
    from waymo_eval_ref import boxes_from_rows

    return boxes_from_rows(rows) if len(rows) else np.zeros((0, 7), np.float32)


def _wide_outputs(tag="wide", with_aux=True):
    z = np.load(os.path.join(HERE, "golden", "render", "panels.npz"))
    head, aux = fixture_panels(z, tag)
    outputs = {"head": {s: {k: (_dev(v) if not isinstance(v, dict) else {"logits": _dev(v["logits"])}) for k, v in level.items()}
                        for s, level in head.items()}}
    if aux is not None and with_aux:
        outputs["aux"] = {s: {t: {k: _dev(v) for k, v in e.items()} for t, e in entries.items()} for s, entries in aux.items()}
    return z, head, aux, outputs


def _frame(rows, scores, batch_index):
    import pyarrow as pa

    tb = _tb()
    return pa.table({**{c: pa.array(np.asarray(rows[:, j], np.float32)) for j, c in enumerate(tb.COLS)},
                     "score": pa.array(np.asarray(scores, np.float32)), "batch_index": pa.array(np.asarray(batch_index, np.int32))})


@pytest.mark.parametrize("variant", ["full", "no_aux", "no_dts", "no_annotations", "max_num_dts"])
def test_draw_detections_two_levels_two_tasks(variant):
    tb = _tb()
    z, head, aux, outputs = _wide_outputs(with_aux=variant != "no_aux")
    ms, mpp = (float(v) for v in z["cfg"])
    ann = torch.from_numpy(z["wide/annotations"])
    dts = _frame(z["wide/dts"], z["wide/dt_scores"], z["wide/dt_batch_index"])
    if variant == "no_dts":
        dts = dts.slice(0, 0)
    if variant == "no_annotations":
        ann = ann[:0]
    rec = {}
    img = tb._draw(dts, {"annotations": ann}, outputs, 3 if variant == "max_num_dts" else 500, ms, mpp, record=rec)
    assert img.is_cuda and img.dtype == torch.uint8
    img = img.cpu().numpy()
    assert np.array_equal(img, _restate(rec, ms, mpp, head[1]["cart"][0]))
    assert rec["kinds"] == [k for _, k, *_ in R.panel_list(head, aux if variant != "no_aux" else None)]
    n_dt0 = int((z["wide/dt_batch_index"] == 0).sum())
    assert len(rec["annotations"]) == (0 if variant == "no_annotations" else 3)
    assert len(rec["detections"]) == {"no_dts": 0, "max_num_dts": 3}.get(variant, n_dt0)
    assert list(rec["scores"]) == sorted(rec["scores"], reverse=True)
    bev = img[:, rec["bev_origin"][0]:, rec["bev_origin"][1]:rec["bev_origin"][1] + rec["side"]]
    if variant == "no_annotations":
        # the detections must NOT be drawn: the image is the reference's (whose polylines are a no-op), bit for bit -- panel layout,
        # both padding branches, colours and the point splat
        assert rec["iou"] is None and np.array_equal(img, z["wide/image"])
    else:
        assert (bev[2] == 255).sum() > (bev[0] == 255).sum()  # blue footprints on top of the white points
        assert (rec["iou"] is None) == (variant == "no_dts")
    if variant == "full":
        assert np.array_equal(tb.draw_detections(dts, None, {"annotations": ann}, outputs, max_side=ms, meter_per_px=mpp).cpu().numpy(), img)
        assert ((bev[0] > 0) & (bev[1] == 0) & (bev[2] == 0)).any()  # a red detection


def test_draw_detections_narrow_layout_equals_the_fixture():
    tb = _tb()
    z, head, aux, outputs = _wide_outputs("narrow")
    ms, mpp = (float(v) for v in z["cfg"])
    img = tb.draw_detections(_frame(z["narrow/dts"], z["narrow/dt_scores"], z["narrow/dt_batch_index"]), None,
                             {"annotations": torch.zeros((0, 13))}, outputs, max_side=ms, meter_per_px=mpp)
    assert np.array_equal(img.cpu().numpy(), z["narrow/image"])


def test_draw_detections_on_the_tiny_models_eval_output(golden):
    from range_view_3d_detection_amd.math.ops.coding import build_dataframe
    from range_view_3d_detection_amd.nn.decoders.range_decoder import RangeDecoder

    tb = _tb()
    t = golden("tiny_model")
    logits, reg, cart, mask = t["eval/logits"], t["eval/regressands"], t["cart"], t["mask"]
    n_cls, B = logits.shape[1], logits.shape[0]
    mo = {1: {"cart": cart.to(DEV), "mask": mask.to(DEV), 0: {"logits": logits.to(DEV), "regressands": reg.to(DEV)}}}
    post = {"num_pre_nms": 50000, "num_post_nms": 40, "nms_threshold": 0.3, "min_confidence": 0.1, "nms_mode": "HARD"}
    names = [f"K{i}" for i in range(n_cls)]
    params, scores, cats, bidx = RangeDecoder(True, False, [], [], []).decode(mo, post, {0: names}, use_nms=True)
    uuids = {"batch_index": list(range(B)), "log_id": [f"log{b}" for b in range(B)], "timestamp_ns": [1000 + b for b in range(B)]}
    dts = build_dataframe(params, scores, cats, bidx, uuids, names)
    pick = torch.arange(0, params.shape[0], 2)
    box = params[pick].double().cpu()
    box[:, :2] += torch.randn(len(pick), 2, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 0.02
    ann = torch.cat([box, torch.zeros(len(pick), 2, dtype=torch.float64), bidx[pick].double().cpu()[:, None]], 1)  # the loader's (M,13) host rows
    ms, mpp = 40.0, 0.25
    rec = {}
    img = tb._draw(dts, {"annotations": ann}, {"head": mo}, 25, ms, mpp, record=rec).cpu().numpy()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # (after the first call: library load, colour tables) nothing waits for the device
    try:
        again = tb.draw_detections(dts, None, {"annotations": ann}, {"head": mo}, max_num_dts=25, max_side=ms, meter_per_px=mpp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.array_equal(again.cpu().numpy(), img)
    n0 = int((bidx == 0).sum())
    assert n0 > 25 and len(rec["detections"]) == 25 and len(rec["annotations"]) == int((bidx[pick] == 0).sum()) > 3
    assert np.array_equal(img, _restate(rec, ms, mpp, cart[0].numpy()))
    H, W = cart.shape[-2:]
    side = R.bev_side(ms, mpp)
    assert img.shape == (3, 3 * H + side, max(W, side)) and rec["kinds"] == ["likelihood", "range", "likelihood"]
    best = rec["iou"].cpu().numpy().max(1)
    assert (best >= 0.7).any(), "a detection beside its own perturbed copy is green"


# ---- compat.mmcv_ops.box_iou_rotated ------------------------------------------------------------------------------------------------
def test_box_iou_rotated_against_the_oracle():
    from oracle import nms as onms
    from range_view_3d_detection_amd import _lib as L
    from range_view_3d_detection_amd.compat.mmcv_ops import box_iou_rotated

    g = np.random.default_rng(31)
    b7 = _random_boxes(g, 150, 12.0)
    a = np.stack([b7[:, 0], b7[:, 1], b7[:, 3], b7[:, 4], b7[:, 6]], 1)  # (cx, cy, w, h, a)
    b = a[::-1].copy()
    b[:75] = a[:75] + (g.standard_normal((75, 5)) * 0.2).astype(np.float32)

    def rect(x):
        half = x[:, 2:4] / np.float32(2)
        return np.concatenate([x[:, :2] - half, x[:, :2] + half, x[:, 4:5]], 1).astype(np.float32)

    want = onms.pairwise_iou(rect(a), rect(b))
    dense = box_iou_rotated(_dev(a), _dev(b)).cpu().numpy()
    assert dense.shape == (150, 150) and np.array_equal(_bits(dense), _bits(want)) and (want > 0.3).sum() > 50
    aligned = box_iou_rotated(_dev(a), _dev(b), aligned=True).cpu().numpy()
    assert aligned.shape == (150,) and np.array_equal(_bits(aligned), _bits(np.diagonal(dense)))
    with pytest.raises(NotImplementedError):
        box_iou_rotated(_dev(a), _dev(b), mode="iof")
    with pytest.raises(NotImplementedError):
        box_iou_rotated(_dev(a), _dev(b), clockwise=False)
    with pytest.raises(L.RvError):
        box_iou_rotated(_dev(a), _dev(b[:10]), aligned=True)
    with pytest.raises(L.RvError):
        box_iou_rotated(torch.from_numpy(a), _dev(b))
