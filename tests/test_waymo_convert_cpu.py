"""The Waymo range-image -> sweep conversion without a GPU: the NumPy restatement of the declared semantics (``tests/waymo_convert_ref.py``)
against an independently written inverse and against hand-worked cases, the host helpers of ``converters/waymo``, the words of
``include/rv3d.h`` that pin the semantics, and the C ABI's argument checks (nothing is launched)."""

from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch

import waymo_convert_ref as ref


@pytest.mark.parametrize("offset", [0.0, 1e3, 1e5])
def test_restatement_against_the_independent_inverse(offset):
    """Forward (fp64, before the final rounding), then back through the frame pose, the transposed pixel pose and the transposed
    extrinsic: the recovered range, azimuth x range and inclination x range are the pixel's to 1e-8 m, also 1e5 m from the origin."""
    f = ref.make_frames(7, 1, 64, 2650, offset=offset)
    _, _, valid, pts = ref.convert(f["range_image"], f["extrinsic"], f["inclination"], f["pixel_pose"], f["frame_pose"])
    rng, az, incl = ref.invert(pts, f["extrinsic"], f["pixel_pose"], f["frame_pose"])
    want_rng = f["range_image"][..., 0].astype(np.float64)
    want_az = np.broadcast_to(ref.azimuths(f["extrinsic"], 2650)[:, None, :], rng.shape)
    want_incl = np.broadcast_to(f["inclination"][:, :, None], rng.shape)
    d_az = (az - want_az + np.pi) % (2 * np.pi) - np.pi
    errs = [np.abs(rng - want_rng)[valid].max(), np.abs(d_az * want_rng)[valid].max(), np.abs((incl - want_incl) * want_rng)[valid].max()]
    print(f"offset {offset:g}: range {errs[0]:.2e} m, azimuth x range {errs[1]:.2e} m, inclination x range {errs[2]:.2e} m")
    assert valid.sum() > 0.5 * valid.size and max(errs) <= 1e-8, errs


def test_restatement_without_a_pixel_pose_inverts_too():
    f = ref.make_frames(8, 2, 16, 250, pixel_pose=False, beam_table=False)
    _, _, valid, pts = ref.convert(f["range_image"], f["extrinsic"], f["inclination"])
    rng, az, incl = ref.invert(pts, f["extrinsic"])
    want = f["range_image"][..., 0].astype(np.float64)
    d_az = (az - ref.azimuths(f["extrinsic"], 250)[:, None, :] + np.pi) % (2 * np.pi) - np.pi
    assert np.abs(rng - want)[valid].max() <= 1e-8 and np.abs(d_az * want)[valid].max() <= 1e-8
    assert np.abs((incl - f["inclination"][:, :, None]) * want)[valid].max() <= 1e-8


def _tiny(range_value=10.0):
    ri = np.zeros((1, 1, 4, 4), np.float32)
    ri[..., 0] = range_value
    ri[..., 1] = [0.25, 0.5, 0.75, 1.0]
    ri[..., 2] = [0.1, 0.2, 0.3, 0.4]
    ri[..., 3] = -1.0
    return ri, np.eye(4)[None].copy(), np.zeros((1, 1))


R2 = math.sqrt(50.0)  # 10 / sqrt(2) = 7.0710678...
IDENTITY_XYZ = np.array([[-R2, R2, 0.0], [R2, R2, 0.0], [R2, -R2, 0.0], [-R2, -R2, 0.0]])


def test_hand_worked_identity_yaw_and_translation():
    ri, E, incl = _tiny()
    sweep, num_pts, valid, pts = ref.convert(ri, E, incl)
    assert abs(R2 - 7.0710678) < 1e-7 and np.abs(pts[0, 0] - IDENTITY_XYZ).max() <= 1e-9  # column 0 is azimuth +3/4 pi: (-, +)
    assert num_pts.tolist() == [4] and valid.all()
    assert np.array_equal(sweep[0, 0, :, :3], ri[0, 0, :, :3]) and np.array_equal(sweep[0, 0, :, 3:], IDENTITY_XYZ.astype(np.float32))
    # an extrinsic that is a pure yaw: the azimuth correction and the rotation cancel
    for yaw in (0.3, -2.5):
        Ey = E.copy()
        Ey[0, :3, :3] = ref._rot("z", np.float64(yaw))
        assert np.abs(ref.convert(ri, Ey, incl)[3][0, 0] - IDENTITY_XYZ).max() <= 1e-9
    # a pure translation shifts them
    Et = E.copy()
    Et[0, :3, 3] = [1.5, -0.25, 2.0]
    assert np.abs(ref.convert(ri, Et, incl)[3][0, 0] - (IDENTITY_XYZ + [1.5, -0.25, 2.0])).max() <= 1e-9
    # inclination: z = range sin(incl), the horizontal part shrinks by cos(incl)
    up = ref.convert(ri, E, np.full((1, 1), 0.2))[3][0, 0]
    assert np.abs(up[:, 2] - 10 * math.sin(0.2)).max() <= 1e-9 and np.abs(up[:, :2] - IDENTITY_XYZ[:, :2] * math.cos(0.2)).max() <= 1e-9


def test_hand_worked_pixel_pose_equal_to_the_frame_pose_is_the_identity():
    ri, E, incl = _tiny()
    E[0, :3, :3] = ref._rot("z", np.float64(0.4)) @ ref._rot("y", np.float64(0.01))
    E[0, :3, 3] = [1.4, 0.0, 2.2]
    pose = np.array([0.02, -0.015, 1.1, 1234.5, -987.25, 12.0], np.float32)
    pp = np.broadcast_to(pose, (1, 1, 4, 6)).copy()
    p64 = pose.astype(np.float64)  # the frame pose built from the pixel pose's fp32 values
    F = np.eye(4)[None].copy()
    F[0, :3, :3] = ref._rot("z", p64[2]) @ ref._rot("y", p64[1]) @ ref._rot("x", p64[0])
    F[0, :3, 3] = p64[3:]
    plain = ref.convert(ri, E, incl)[3]
    posed = ref.convert(ri, E, incl, pp, F)[3]
    assert np.abs(posed - plain).max() <= 1e-9
    # a pixel pose 1 m ahead of the frame pose along the vehicle's x moves the point by +1 m in x
    ahead = pp.copy()
    ahead[..., 3:] = (p64[3:] + F[0, :3, :3] @ [1.0, 0.0, 0.0]).astype(np.float32)
    moved = ref.convert(ri, E, incl, ahead, F)[3]
    assert np.abs(moved - (plain + [1.0, 0.0, 0.0])).max() <= 2e-4  # (the fp32 rounding of the 1e3 m translation: 6e-5 m per axis)


def test_hand_worked_invalid_pixels_are_zero_rows():
    ri, E, incl = _tiny()
    ri[0, 0, 0, 0] = -1.0
    ri[0, 0, 1, 0] = np.nan
    ri[0, 0, 2, 3] = 1.0
    pp = np.zeros((1, 1, 4, 6), np.float32)
    pp[0, 0, 2] = np.nan  # a NaN pose at an invalid pixel leaves zeros (a select, not a product)
    for args in ((), (pp, np.eye(4)[None])):
        sweep, num_pts, valid, _ = ref.convert(ri, E, incl, *args)
        assert valid[0, 0].tolist() == [False, False, False, True] and num_pts.tolist() == [1]
        assert np.array_equal(sweep[0, 0, :3], np.zeros((3, 6), np.float32)) and not np.signbit(sweep[0, 0, :3]).any()
        assert np.array_equal(sweep[0, 0, 3], np.array([10.0, 1.0, 0.4, -R2, -R2, 0.0], np.float32))
    with pytest.raises(ValueError):
        ref.convert(ri, E, incl, None, np.eye(4)[None])


def test_fp32_chain_differs_from_fp64_by_millimetres_far_from_the_origin():
    """The documented distance between the fp64 yardstick and the TensorFlow-like fp32 reading; not a bound on the kernel."""
    out = {}
    for offset in (0.0, 1e4, 1e5):
        f = ref.make_frames(11, 1, 16, 500, offset=offset)
        args = (f["range_image"], f["extrinsic"], f["inclination"], f["pixel_pose"], f["frame_pose"])
        _, _, valid, p64 = ref.convert(*args)
        p32 = ref.convert(*args, dtype=np.float32)[3]
        out[offset] = float(np.abs(p32.astype(np.float64) - p64)[valid].max())
    print({k: f"{v:.2e} m" for k, v in out.items()})
    # fp32 carries 6e-8 of the magnitude per operation: a few of them on 1e4 / 1e5 m; five orders above the fp64 chain's 3e-11 m either way
    assert out[0.0] < 1e-4 and 1e-4 < out[1e4] < 2e-2 and 1e-3 < out[1e5] < 2e-1


def test_inclination_helpers():
    from range_view_3d_detection_amd._lib import RvError
    from range_view_3d_detection_amd.converters import waymo as W

    assert np.allclose(W.compute_inclination(-0.3, 0.1, 4), [-0.25, -0.15, -0.05, 0.05], rtol=0, atol=1e-15)
    assert np.allclose(W.inclinations_by_row(4, [], -0.3, 0.1), [0.05, -0.05, -0.15, -0.25], rtol=0, atol=1e-15)
    assert np.allclose(W.inclinations_by_row(4, None, -0.3, 0.1), [0.05, -0.05, -0.15, -0.25], rtol=0, atol=1e-15)
    assert W.inclinations_by_row(3, [-0.3, -0.1, 0.02], 9.0, 9.0).tolist() == [0.02, -0.1, -0.3]  # the table wins, reversed
    assert W.compute_inclination(-0.3, 0.1, 4).dtype == np.float64 and W.inclinations_by_row(3, [1, 2, 3]).flags["C_CONTIGUOUS"]
    for h in (1, 5, 64):
        assert np.array_equal(W.compute_inclination(-0.31, 0.04, h), ref.compute_inclination(-0.31, 0.04, h))
        assert np.array_equal(W.inclinations_by_row(h, None, -0.31, 0.04), ref.inclinations_by_row(h, None, -0.31, 0.04))
    with pytest.raises(RvError, match="beam inclinations"):
        W.inclinations_by_row(4, [0.1, 0.2])
    with pytest.raises(RvError, match="beam_inclination_min"):
        W.inclinations_by_row(4)


def test_labels_to_annotations():
    from range_view_3d_detection_amd.converters.waymo import labels_to_annotations
    from range_view_3d_detection_amd.converters.waymo.utils import ANNOTATION_COLUMNS
    from range_view_3d_detection_amd.prototype.loader import annotations_for_sweep

    labels = {"type": [1, 3, 2, 0, 4], "center_x": [10.0, 1.0, -5.0, 2.0, 7.5], "center_y": [2.0, 1.0, 4.0, 2.0, -3.0], "center_z": [0.5, 1.0, 0.9, 2.0, 0.8],
              "length": [4.5, 0.3, 0.8, 1.0, 1.8], "width": [2.0, 0.3, 0.7, 1.0, 0.8], "height": [1.6, 2.0, 1.8, 1.0, 1.7],
              "heading": [math.pi / 2, 0.0, -0.4, 0.0, 3.0], "num_lidar_points_in_box": [120, 4, 3, 9, 0], "detection_difficulty_level": [0, 0, 2, 0, 1],
              "id": ["a", "b", "c", "d", "e"]}
    t = labels_to_annotations(labels, 1550083467346370)
    assert tuple(t.column_names) == ANNOTATION_COLUMNS and t.num_rows == 3  # SIGN and UNKNOWN dropped
    assert t.column("category").to_pylist() == ["VEHICLE", "PEDESTRIAN", "CYCLIST"] and t.column("track_uuid").to_pylist() == ["a", "c", "e"]
    assert t.column("timestamp_ns").to_pylist() == [1550083467346370] * 3
    assert abs(t.column("qw")[0].as_py() - math.sqrt(0.5)) < 1e-15 and abs(t.column("qz")[0].as_py() - math.sqrt(0.5)) < 1e-15
    assert t.column("qx").to_pylist() == [0.0] * 3 == t.column("qy").to_pylist()
    assert abs(t.column("qw")[1].as_py() - math.cos(-0.2)) < 1e-15 and abs(t.column("qz")[1].as_py() - math.sin(-0.2)) < 1e-15
    assert t.column("num_interior_pts").to_pylist() == [120, 3, 0] and t.column("difficulty_level").to_pylist() == [0, 2, 1]
    assert t.column("tx_m").to_pylist() == [10.0, -5.0, 7.5] and t.column("length_m").to_pylist() == [4.5, 0.8, 1.8]
    assert labels_to_annotations(labels, 5, log_id="seg").column("log_id").to_pylist() == ["seg"] * 3
    # it feeds the loader's annotation step as it is: rows with interior points, in task order
    rows = annotations_for_sweep(t, 1550083467346370, {0: ["VEHICLE"], 1: ["PEDESTRIAN", "CYCLIST"]}, batch_index=2)
    assert rows.shape == (2, 13) and rows[:, 0].tolist() == [10.0, -5.0] and rows[:, 10].tolist() == [0.0, 1.0] and rows[:, 11].tolist() == [0.0, 1.0]
    assert rows[:, 12].tolist() == [2.0, 2.0] and abs(float(rows[0, 9]) - math.sqrt(0.5)) < 1e-15
    empty = labels_to_annotations({k: [] for k in labels}, 5)
    assert empty.num_rows == 0 and annotations_for_sweep(empty, 5, {0: ["VEHICLE"]}).shape == (0, 13)


SYMBOLS = ("rv_waymo_range_image_to_sweep", "rv_waymo_range_image_to_batch")


def test_header_pins_the_semantics_and_both_builds_export_the_entries():
    from range_view_3d_detection_amd import _lib as L

    assert set(SYMBOLS) <= set(L.declared_symbols())
    for tag in ("bf16", "f16"):
        lib = L.load(tag)
        for name in SYMBOLS:
            assert hasattr(lib, name), (tag, name)
    header = open(L.HEADER_PATH).read()
    section = header[header.index("Waymo range image -> sweep"):]
    for words in ("ratio = (W - c - 0.5) / W", "(2 ratio - 1) pi - az_correction", "atan2(E[1][0], E[0][0])", "SELECT", "fp64", "rounded to fp32 once",
                  "Rz(yaw) Ry(pitch) Rx(roll)", "nlz != 1.0", "NOT\n * pinned", "num_pts"):
        assert words in section, words


def test_argument_checks_reject_before_anything_is_launched():
    from range_view_3d_detection_amd import _lib as L

    lib = L.load()
    buf = (ctypes.c_int64 * 64)()  # (a host buffer: only ever checked for null / alignment, never dereferenced by a rejected call)
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    src, op = (ctypes.c_int32 * 17)(*([2, 1, 0, 3, 4, 5] + [0] * 11)), (ctypes.c_int32 * 17)(*([0, 1] + [0] * 15))

    def rejected(name, args, match):
        assert getattr(lib, name)(*args) == 1, (name, match)
        assert match in lib.rv_last_error().decode(), lib.rv_last_error()

    def common(k):
        return [k.get("ri", p), k.get("ext", p), k.get("incl", p), k.get("pp", null), k.get("inv", null), k.get("B", 1), k.get("H", 2),
                k.get("W", 8)]

    sweep = lambda **k: common(k) + [k.get("sweep", p), k.get("num_pts", p), null]
    batch = lambda **k: common(k) + [k.get("n_feat", 6), k.get("src", src), k.get("op", op), k.get("pad", 3), k.get("circular", 0),
                                     k.get("features", p), k.get("cart", p), k.get("mask", p), k.get("num_pts", p), null]
    for name, make in (("rv_waymo_range_image_to_sweep", sweep), ("rv_waymo_range_image_to_batch", batch)):
        rejected(name, make(ri=null), "null")
        rejected(name, make(ext=null), "null")
        rejected(name, make(incl=null), "null")
        rejected(name, make(B=0), "empty")
        rejected(name, make(H=-1), "empty")
        rejected(name, make(W=0), "empty")
        rejected(name, make(B=65536), "launch grid")
        rejected(name, make(H=70000), "launch grid")
        rejected(name, make(pp=p), "go together")
        rejected(name, make(inv=p), "go together")
        rejected(name, make(ri=odd), "aligned")
        rejected(name, make(pp=odd, inv=p), "aligned")
    rejected("rv_waymo_range_image_to_sweep", sweep(sweep=null), "sweep")
    rejected("rv_waymo_range_image_to_sweep", sweep(sweep=odd), "sweep")
    b = "rv_waymo_range_image_to_batch"
    for key in ("features", "cart", "mask", "src", "op"):
        rejected(b, batch(**{key: null}), "null")
    rejected(b, batch(n_feat=0), "features (1..16)")
    rejected(b, batch(n_feat=17), "features (1..16)")
    rejected(b, batch(pad=-1), "pad")
    rejected(b, batch(src=(ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 6)), "not a sweep channel")
    rejected(b, batch(src=(ctypes.c_int32 * 6)(0, -1, 2, 3, 4, 5)), "not a sweep channel")
    rejected(b, batch(op=(ctypes.c_int32 * 6)(0, 2, 0, 0, 0, 0)), "op 2")


def test_cpu_tensors_and_bad_shapes_raise():
    from range_view_3d_detection_amd._lib import RvError
    from range_view_3d_detection_amd.converters import waymo as W

    ri, ext, incl = torch.zeros(2, 4, 8, 4), torch.eye(4).repeat(2, 1, 1), torch.zeros(2, 4)
    cfg = {"height": 4, "width": 8, "feature_column_names": list(ref.WAYMO_FEATURES)}
    with pytest.raises(RvError, match="no CPU fallback"):
        W.range_image_to_sweep(ri, ext, incl)
    with pytest.raises(RvError, match="no CPU fallback"):
        W.batch_from_range_images(ri, ext, incl, None, None, cfg)
    with pytest.raises(RvError, match="one frame"):
        W.sweep_table(torch.zeros(2, 4, 8, 6))
    table = W.sweep_table(torch.arange(4 * 8 * 6, dtype=torch.float32).reshape(4, 8, 6))
    assert tuple(table) == ref.TABLE_COLUMNS and all(c.shape == (32,) and c.dtype == np.float32 for c in table.values())
    assert table["x"][:2].tolist() == [3.0, 9.0] and table["range"][:2].tolist() == [0.0, 6.0] and table["elongation"][1] == 8.0
