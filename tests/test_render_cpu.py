"""The debug panels without a GPU: the NumPy restatement (``tests/render_ref.py``) against the reference's own functions
(``tests/golden/render/*.npz``, made by ``tests/golden/make_golden_render.py``) and against hand-worked raster cases
(``tests/golden/render_cases.json``); the colour tables against matplotlib; the entries' declarations, exports and declared-semantics
text; ``to_logger`` with fake trainer and logger objects."""

from __future__ import annotations

import importlib.util
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import render_ref as R  # noqa: E402
from range_view_3d_detection_amd import _lib as L  # noqa: E402

RENDER_HEADER = os.path.join(ROOT, "include", "rv3d_render.h")
ENTRIES = ("rv_render_colormap_table", "rv_render_plane", "rv_render_colormap", "rv_render_bev_points", "rv_render_bev_boxes", "rv_boxes_iou3d",
           "rv_rotated_iou_pairs")


def _npz(name):
    return np.load(os.path.join(HERE, "golden", "render", name + ".npz"))


def _cases():
    with open(os.path.join(HERE, "golden", "render_cases.json")) as f:
        return json.load(f)


def _expected_set(case):
    pix = {tuple(p) for p in case.get("pixels", [])}
    for r0, r1, c0, c1 in case.get("rects", []):
        pix |= {(r, c) for r in range(r0, r1 + 1) for c in range(c0, c1 + 1)}
    return pix


def fixture_panels(z, tag):
    """The fixture's network outputs as numpy: (head, aux or None) with the dict order the generator used."""
    head, aux = {}, {}
    tasks = [int(t) for t in z[f"{tag}/tasks"]]
    for s in (int(s) for s in z[f"{tag}/strides"]):
        head[s] = {"cart": z[f"{tag}/head/{s}/cart"], "mask": z[f"{tag}/head/{s}/mask"]}
        for t in tasks:
            head[s][t] = {"logits": z[f"{tag}/head/{s}/{t}/logits"]}
        if len(z[f"{tag}/aux_keys"]) and s == 1:
            aux[s] = {t: {str(k): z[f"{tag}/aux/{s}/{t}/{k}"] for k in z[f"{tag}/aux_keys"]} for t in tasks}
    return head, (aux or None)


def restated_image(head, aux, max_side, mpp, tables, planes=None):
    """The stacked image of sample 0 without boxes, planes by NumPy (or the given ones)."""
    rgb, kinds = [], []
    for i, (stride, kind, t, k, ch) in enumerate(R.panel_list(head, aux)):
        level = head[stride]
        if planes is not None:
            plane = planes[i]
        elif kind == "range":
            plane = R.plane_norm(level["cart"][0])
        elif kind == "likelihood":
            plane = R.plane_likelihood(level[t]["logits"][0])
        else:
            plane = R.plane_abs(aux[stride][t][k][0, ch])
        rgb.append(R.normalize_apply_colormap(plane, tables["TURBO_R" if kind == "range" else "VIRIDIS"], level["mask"][0, 0]))
        kinds.append(kind)
    return R.stack(rgb, kinds, R.bev_points(head[1]["cart"][0], max_side, mpp))


# ---- the restatement against the reference ---------------------------------------------------------------------------------------
def test_restated_colormap_equals_the_reference():
    z = _npz("functions")
    mask = z["colormap/mask"]
    n = 0
    for key in z.files:
        m = re.fullmatch(r"colormap/(\w+)/(GREYS|TURBO_R|VIRIDIS)/(\w+)", key)
        if not m:
            continue
        plane, table = z[f"colormap/{m.group(1)}/plane"], z[f"tables/{m.group(2)}"]
        msk = {"masked": mask, "all_masked": np.zeros_like(mask), "unmasked": None}[m.group(3)]
        assert np.array_equal(R.normalize_apply_colormap(plane, table, msk), z[key]), key
        n += 1
    assert n == 27
    assert not z["colormap/random/VIRIDIS/all_masked"].any()
    assert (R.colormap_index(z["colormap/constant/plane"]) == 0).all()
    idx = R.colormap_index(z["colormap/single_max/plane"])
    assert idx[3, 17] == 254 and idx.sum() == 254  # (7 / (7 + 1e-6) * 255 stays below 255)


def test_restated_point_splat_equals_the_reference():
    z = _npz("functions")
    max_side, mpp = (float(v) for v in z["cfg"])
    xyz = z["points/xyz"]
    assert R.bev_side(max_side, mpp) == 40 and R.bev_side(75.0, 0.15) == 1000
    assert np.array_equal(R.bev_points(xyz.T, max_side, mpp).transpose(1, 2, 0), z["points/bev"])
    # world_to_image: the reference filters the rows and replaces x, y by the pixel; z stays
    (kx, r), (ky, c) = R.world_to_image(xyz[:, 0], max_side, mpp), R.world_to_image(xyz[:, 1], max_side, mpp)
    keep = kx & ky
    assert np.array_equal(np.stack([r[keep], c[keep], xyz[keep, 2]], 1), z["points/world_to_image"])


@pytest.mark.parametrize("tag", ["wide", "narrow"])
def test_restated_panels_equal_the_reference(tag):
    z, f = _npz("panels"), _npz("functions")
    max_side, mpp = (float(v) for v in z["cfg"])
    head, aux = fixture_panels(z, tag)
    tables = {k: f[f"tables/{k}"] for k in ("GREYS", "TURBO_R", "VIRIDIS")}
    img = restated_image(head, aux, max_side, mpp, tables)
    assert img.shape == z[f"{tag}/image"].shape
    assert np.array_equal(img, z[f"{tag}/image"])


def test_layout_of_the_package_equals_the_restatement_and_the_fixture():
    from range_view_3d_detection_amd.rendering import tensorboard as tb

    z = _npz("panels")
    for tag, n_panels, width, bev_col in (("wide", 14, 64, 12), ("narrow", 3, 40, 0)):
        head, aux = fixture_panels(z, tag)
        sizes = [("range" if kind == "range" else kind, 4, head[s]["cart"].shape[-1]) for s, kind, *_ in R.panel_list(head, aux)]
        assert len(sizes) == n_panels
        got = tb.compose(sizes, 40)
        assert got == R.compose(sizes, 40)
        assert (got[0], got[1]) == z[f"{tag}/image"].shape[1:] and got[1] == width and got[3] == (4 * n_panels, bev_col)
    # narrow: W 37 against 40 -> left 1 (right 2); wide, level 2: W 32 against the view padded to 64 -> left 16
    assert tb.compose([("range", 4, 37)], 40)[2] == [(0, 1)]
    assert tb.compose([("range", 4, 64), ("range", 4, 32)], 40)[2] == [(0, 0), (4, 16)]
    with pytest.raises(L.RvError):
        tb.compose([("likelihood", 4, 64), ("range", 4, 32)], 40)


# ---- the declared raster rule, hand-worked ---------------------------------------------------------------------------------------
def test_segment_rule_on_hand_worked_cases():
    cases = _cases()
    side = cases["view"]["side"]
    assert [c["name"] for c in cases["segments"]][:4] == ["horizontal", "vertical", "diagonal_45", "zero_length"]
    for c in cases["segments"]:
        got = set(R.segment_pixels(tuple(c["a"]), tuple(c["b"]), side))
        assert got == _expected_set(c), c["name"]
        assert got == set(R.segment_pixels(tuple(c["b"]), tuple(c["a"]), side)), c["name"]  # (the rule is symmetric)


def test_box_cases_hand_worked():
    cases = _cases()
    v = cases["view"]
    ms, mpp, side = v["max_side"], v["meter_per_px"], v["side"]
    assert R.bev_side(ms, mpp) == side
    for c in cases["boxes"]:
        corners = [R.footprint_pixels(b, ms, mpp) for b in c["boxes"]]
        assert corners == [[tuple(p) for p in box] for box in c["corners"]], c["name"]
        bev = np.zeros((3, side, side), np.uint8)
        bev[:, 15, 18] = 255  # a point under the lines
        out = R.draw_boxes(bev, c["boxes"], c["scores"], c["channels"], ms, mpp)
        drawn = {(int(r), int(cc)) for r, cc in np.argwhere((out != bev).any(0))}
        if "rects" in c:
            want = _expected_set(c)
        else:  # (an oblique polyline: the union of its segments by the rule, through the hand-worked corners)
            want = {p for box in corners for a, b in zip(box[:-1], box[1:]) for p in R.segment_pixels(a, b, side)}
        assert drawn == want, c["name"]
        for r, cc, rgb in c["probes"]:
            assert out[:, r, cc].tolist() == rgb, (c["name"], r, cc)
    assert R.box_value(0.5) == 128 and R.box_value(1.0) == 255 and R.box_value(0.83) == 212 and R.box_value(2.0) == 255


def test_on_segment_equals_its_overflow_free_form():
    """The kernel evaluates the three cases of the declared inequality divided by L2; here both forms on every pixel of small views."""
    rng = np.random.default_rng(5)
    for _ in range(60):
        a, b = (tuple(int(v) for v in rng.integers(-2, 14, 2)) for _ in range(2))
        for r in range(-3, 16):
            for c in range(-3, 16):
                dr, dc, er, ec = b[0] - a[0], b[1] - a[1], r - a[0], c - a[1]
                L2, s = dr * dr + dc * dc, er * dr + ec * dc
                if L2 == 0 or s <= 0:
                    fast = er * er + ec * ec <= 1
                elif s >= L2:
                    fast = (r - b[0]) ** 2 + (c - b[1]) ** 2 <= 1
                else:
                    fast = (er * dc - ec * dr) ** 2 <= L2
                assert fast == R.on_segment((r, c), a, b)


# ---- colour tables ----------------------------------------------------------------------------------------------------------------
def _gen_colormaps():
    spec = importlib.util.spec_from_file_location("gen_colormaps", os.path.join(ROOT, "range_view_3d_detection_amd", "csrc", "gen_colormaps.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_colormaps_header_regenerates_from_matplotlib():
    pytest.importorskip("matplotlib")
    with open(os.path.join(ROOT, "range_view_3d_detection_amd", "csrc", "colormaps.h")) as f:
        assert f.read() == _gen_colormaps().header_text()


def test_library_tables_equal_the_reference_tables():
    from range_view_3d_detection_amd.rendering import tensorboard as tb

    z = _npz("functions")
    for name in ("GREYS", "TURBO_R", "VIRIDIS"):
        t = getattr(tb, name)
        assert t.dtype == torch.uint8 and tuple(t.shape) == (3, 256) and not t.is_cuda
        assert np.array_equal(t.numpy(), z[f"tables/{name}"]), name
    with pytest.raises(AttributeError):
        tb.NO_SUCH_TABLE


# ---- declarations -----------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_exported_by_both_builds():
    protos = L.companion_prototypes()
    assert sorted(protos) == sorted(ENTRIES) and not set(protos) & (set(L.prototypes()) | set(L.included_prototypes()))
    for name in ENTRIES:
        assert name in protos, name
        for tag in ("bf16", "f16"):
            assert hasattr(L.load(tag), name), (tag, name)
    names = [p for _, p in protos["rv_render_bev_boxes"][1]]
    assert names == ["boxes", "scores", "channels", "n", "max_side", "meter_per_px", "side", "zbuf", "image", "H_total", "W_total", "row0", "col0",
                     "stream"]
    assert [p for _, p in protos["rv_boxes_iou3d"][1]] == ["a", "n", "b", "m", "out", "stream"]


def test_header_states_the_declared_semantics():
    text = re.sub(r"\s+", " ", open(RENDER_HEADER).read().replace("\n *", " "))
    for phrase in ("sqrtf((x*x + y*y) + z*z)", "1 / (1 + expf(-max_c logit))", "((x - min) / ((max - min) + 1e-6f)) * 255.0f",
                   "over ALL pixels, masked ones included", "A constant plane maps to index 0",
                   "side = int(math.ceil(max_side * 2 / meter_per_px))", "0 < u < upper", "floorf(size - u)",
                   "corners 6, 2, 3, 7", "the rear edge stays open", "DECLARED raster rule",
                   "|(p - a) * L2 - t * d|^2 <= L2 * L2", "|p - a|^2 <= 1 for L2 == 0", "uint8(rintf(255.0f * score))",
                   "atomicMax of the draw index", "z the box CENTRE", "no text label", "uint8(cmap(i)[:3] * 255.0)"):
        assert phrase in text, phrase
    defines = dict(re.findall(r"#define (RV_(?:PLANE|CMAP)_\w+) (\d+)", open(RENDER_HEADER).read()))
    assert defines == {"RV_PLANE_NORM": "0", "RV_PLANE_LIKELIHOOD": "1", "RV_PLANE_ABS": "2", "RV_PLANE_IDENTITY": "3", "RV_CMAP_GREYS": "0",
                       "RV_CMAP_TURBO_R": "1", "RV_CMAP_VIRIDIS": "2"}


def test_render_is_built_without_contraction():
    mk = open(os.path.join(ROOT, "range_view_3d_detection_amd", "csrc", "Makefile")).read()
    exact = re.search(r"^EXACT\s*:=(.*)$", mk, flags=re.M).group(1).split()
    assert "build/render.o" in exact and "build_f16/render.o" in exact
    assert mk.count("colormaps.h") == 2 and mk.count("../../include/rv3d_render.h") == 2


def test_modules_import_without_the_third_party_packages():
    import ast

    import range_view_3d_detection_amd.compat.mmcv_ops as mo
    import range_view_3d_detection_amd.rendering.tensorboard as tb

    for mod in (tb, mo):
        roots = set()
        for node in ast.walk(ast.parse(open(mod.__file__).read())):
            if isinstance(node, ast.Import):
                roots |= {a.name.split(".")[0] for a in node.names}
            elif isinstance(node, ast.ImportFrom) and node.level == 0:
                roots.add(node.module.split(".")[0])
        assert not roots & {"cv2", "kornia", "mmcv", "pytorch_lightning", "lightning", "matplotlib", "polars"}, (mod.__name__, roots)
    for fn in ("normalize_apply_colormap", "build_bev", "world_to_image", "draw_on_bev", "draw_detections", "to_logger", "log_image"):
        assert callable(getattr(tb, fn)), fn
    with pytest.raises(L.RvError):
        mo.boxes_iou3d(torch.zeros(2, 7), torch.zeros(3, 7))
    with pytest.raises(L.RvError):
        mo.box_iou_rotated(torch.zeros(2, 5), torch.zeros(3, 5))
    with pytest.raises(L.RvError):
        tb.build_bev(torch.zeros(4, 3), 3.0, 0.15)


# ---- to_logger ----------------------------------------------------------------------------------------------------------------------
class _Wandb:
    def __init__(self):
        self.calls, self.experiment = [], object()

    def log_image(self, key, images, caption=None):
        self.calls.append((key, images, caption))


class _Tensorboard:
    def __init__(self):
        self.calls = []
        self.experiment = types.SimpleNamespace(add_image=lambda tag, img, global_step=None: self.calls.append((tag, img, global_step)))


def _trainer(logger, stage="train", rank=0, step=7):
    return types.SimpleNamespace(logger=logger, state=types.SimpleNamespace(stage=types.SimpleNamespace(value=stage)), global_rank=rank,
                                 global_step=step)


def test_to_logger_rank_sanity_check_and_both_loggers(monkeypatch):
    from range_view_3d_detection_amd.rendering import tensorboard as tb

    image = torch.arange(3 * 4 * 5, dtype=torch.uint8).reshape(3, 4, 5)
    drawn = []

    def fake_draw(**kw):
        drawn.append(kw)
        return image

    monkeypatch.setattr(tb, "draw_detections", fake_draw)
    uuids = {"log_id": ["a", "b"], "timestamp_ns": [10, 20], "batch_index": [0, 1]}
    args = dict(dts=None, uuids=uuids, data={}, network_outputs={}, tasks_cfg=None, debug=False)

    w = _Wandb()
    tb.to_logger(trainer=_trainer(w, "validate"), batch_index=1, **args)
    assert len(drawn) == 1 and drawn[0]["max_num_dts"] == 100 and drawn[0]["max_side"] == 75.0 and drawn[0]["meter_per_px"] == 0.15
    (key, images, caption), = w.calls
    assert key == "validate" and caption == ["b-20"] and len(images) == 1
    assert images[0].shape == (4, 5, 3) and np.array_equal(images[0], image.numpy().transpose(1, 2, 0))

    t = _Tensorboard()
    tb.to_logger(trainer=_trainer(t, "train", step=9), batch_index=0, **args)
    (tag, img, step), = t.calls
    assert tag == "train/a-10" and step == 9 and img.shape == (3, 4, 5) and np.array_equal(img, image.numpy())

    n = len(drawn)
    tb.to_logger(trainer=_trainer(_Wandb(), "sanity_check"), batch_index=0, **args)  # Lightning's sanity check: nothing
    tb.to_logger(trainer=_trainer(_Wandb(), "train", rank=1), batch_index=0, **args)  # not rank zero: nothing
    assert len(drawn) == n
    tb.to_logger(trainer=_trainer(None), batch_index=0, **args)  # no logger: drawn, logged nowhere
    tb.log_image("x", image.numpy(), _trainer(object()))  # an unknown logger: nothing, no error
