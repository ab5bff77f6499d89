"""Waymo range image -> sweep on the device -- replaces the reference's offline exporter ``converters/waymo/export.py``
(``convert_range_image_to_cartesian`` ``:55-147``, ``export_sweep`` ``:255-285``, ``export_annotations`` ``:415-501``).

The reference runs TensorFlow and ``waymo_open_dataset`` once per frame on the host and stores a feather table; here the polar ->
vehicle-frame step is one HIP launch per batch (``csrc/waymo_sweep.hip``), so frames can be converted online, right in front of the
detector.  Neither library is available to this project: the arithmetic is DECLARED in ``include/rv3d.h`` and not
pinned against their binaries.  It runs in fp64 and rounds once, where TensorFlow computes in fp32.

* :func:`compute_inclination`, :func:`inclinations_by_row` -- the per-row inclinations from the calibration (``export.py:103-112``);
* :func:`range_image_to_sweep` -- ``rv_waymo_range_image_to_sweep``: the reference's table as a (B, H, W, 6) tensor, and ``num_pts``;
* :func:`sweep_table`, :func:`write_sweep` -- that tensor as the column dict / feather file the loader reads;
* :func:`batch_from_range_images` -- ``rv_waymo_range_image_to_batch``: straight to the detector's (padded) batch dict;
* :func:`labels_to_annotations` -- the label rows (host work on a handful of rows).

Only the first return of the top lidar is converted (all the reference exports, ``:97-98, 262-270``).  Reading TFRecord / Parquet
files into arrays stays with the caller.  No CPU fallback.
"""

from __future__ import annotations

import ctypes
from typing import Any, Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from ... import _lib as L
from ...engine import _require_cuda
from ...prototype.loader import _PAD

SWEEP_CHANNELS = ("range", "intensity", "elongation", "x", "y", "z")  # channel order of the sweep tensor (export.py:140-146)
TABLE_COLUMNS = ("x", "y", "z", "range", "intensity", "elongation")  # column order of the exported table (export.py:272-276)
LABEL_TYPES = ("UNKNOWN", "VEHICLE", "PEDESTRIAN", "SIGN", "CYCLIST")  # waymo_open_dataset.label_pb2.Label.Type
ANNOTATION_COLUMNS = ("timestamp_ns", "track_uuid", "category", "length_m", "width_m", "height_m", "qw", "qx", "qy", "qz", "tx_m", "ty_m", "tz_m",
                      "num_interior_pts", "difficulty_level")  # export.py:438-454


def compute_inclination(inclination_min: float, inclination_max: float, height: int) -> np.ndarray:
    """``range_image_utils.compute_inclination``: ``(r + 0.5) / height * (max - min) + min`` for r = 0 .. height-1 (ascending), fp64."""
    r = np.arange(int(height), dtype=np.float64)
    return (r + 0.5) / float(height) * (float(inclination_max) - float(inclination_min)) + float(inclination_min)


def inclinations_by_row(height: int, beam_inclinations=None, beam_inclination_min: Optional[float] = None,
                        beam_inclination_max: Optional[float] = None) -> np.ndarray:
    """Inclination of every IMAGE ROW (row 0 = the highest beam), fp64: the calibration's beam table reversed (``export.py:109``), or, when
    the table is empty, :func:`compute_inclination` of the calibration's min / max, reversed."""
    if beam_inclinations is not None and len(beam_inclinations) > 0:
        incl = np.asarray(beam_inclinations, dtype=np.float64).reshape(-1)
        if incl.shape[0] != int(height):
            raise L.RvError(f"{incl.shape[0]} beam inclinations for an image of {height} rows")
    else:
        if beam_inclination_min is None or beam_inclination_max is None:
            raise L.RvError("inclinations_by_row: an empty beam table needs beam_inclination_min and beam_inclination_max")
        incl = compute_inclination(beam_inclination_min, beam_inclination_max, height)
    return np.ascontiguousarray(incl[::-1])


def _inputs(range_image, extrinsic, inclination, pixel_pose, frame_pose):
    """Batched, contiguous device tensors of the kernel's inputs; the inverse frame pose is formed on the host in fp64."""
    _require_cuda(range_image, "range_image")
    dev = range_image.device
    single = range_image.dim() == 3
    ri = (range_image[None] if single else range_image).float().contiguous()
    if ri.dim() != 4 or ri.shape[-1] != 4:
        raise L.RvError(f"range_image has shape {tuple(range_image.shape)}, expected (H, W, 4) or (B, H, W, 4): range, intensity, elongation, nlz")
    b, h, w, _ = ri.shape
    ext = torch.as_tensor(extrinsic).to(dev, torch.float64).reshape(-1, 4, 4).contiguous()
    inc = torch.as_tensor(inclination).to(dev, torch.float64).reshape(-1, h).contiguous()
    if ext.shape[0] != b or inc.shape[0] != b:
        raise L.RvError(f"{b} range images, {ext.shape[0]} extrinsics, {inc.shape[0]} inclination rows")
    if (pixel_pose is None) != (frame_pose is None):
        raise L.RvError("pixel_pose and frame_pose go together: a per-pixel pose needs the pose of the frame, and the reverse")
    pp = inv = None
    if pixel_pose is not None:
        pp = (pixel_pose[None] if pixel_pose.dim() == 3 else pixel_pose).to(dev, torch.float32).contiguous()
        if tuple(pp.shape) != (b, h, w, 6):
            raise L.RvError(f"pixel_pose has shape {tuple(pixel_pose.shape)}, expected {(b, h, w, 6)}: roll, pitch, yaw, tx, ty, tz")
        fp = torch.as_tensor(frame_pose).detach().cpu().to(torch.float64).reshape(-1, 4, 4).numpy()
        if fp.shape[0] != b:
            raise L.RvError(f"{b} range images, {fp.shape[0]} frame poses")
        inv = torch.from_numpy(np.ascontiguousarray(np.linalg.inv(fp)[:, :3, :])).to(dev)
    return single, ri, ext, inc, pp, inv


def range_image_to_sweep(range_image: Tensor, extrinsic, inclination, pixel_pose: Optional[Tensor] = None, frame_pose=None) -> Tuple[Tensor, Tensor]:
    """``range_image`` (B, H, W, 4) fp32 [range, intensity, elongation, nlz] (or one frame (H, W, 4)), ``extrinsic`` (B, 4, 4) vehicle <-
    sensor, ``inclination`` (B, H) by image row (:func:`inclinations_by_row`), ``pixel_pose`` (B, H, W, 6) [roll, pitch, yaw, tx, ty, tz]
    with ``frame_pose`` (B, 4, 4), or neither -> (``sweep`` (B, H, W, 6) fp32 [range, intensity, elongation, x, y, z], zeros where there
    is no return or a no-label zone; ``num_pts`` (B,) int64 valid pixels).  One launch; asynchronous."""
    single, ri, ext, inc, pp, inv = _inputs(range_image, extrinsic, inclination, pixel_pose, frame_pose)
    b, h, w, _ = ri.shape
    sweep = torch.empty((b, h, w, 6), dtype=torch.float32, device=ri.device)
    num_pts = torch.empty(b, dtype=torch.int64, device=ri.device)
    with torch.cuda.device(ri.device):
        L.call("rv_waymo_range_image_to_sweep", L.ptr(ri), L.ptr(ext), L.ptr(inc), L.ptr(pp), L.ptr(inv), b, h, w,
               L.ptr(sweep), L.ptr(num_pts), L.stream_ptr())
    return (sweep[0], num_pts[0]) if single else (sweep, num_pts)


def sweep_table(sweep: Tensor) -> Dict[str, np.ndarray]:
    """One frame's sweep (H, W, 6) -> the exported table: ``x, y, z, range, intensity, elongation`` (``export.py:272-276``), H*W fp32 rows
    each -- what ``prototype.loader.range_view_from_table`` takes.  Reads the sweep back to the host."""
    if sweep.dim() != 3 or sweep.shape[-1] != 6:
        raise L.RvError(f"sweep has shape {tuple(sweep.shape)}, expected (H, W, 6): one frame")
    host = sweep.detach().float().reshape(-1, 6).cpu().numpy()
    return {name: np.ascontiguousarray(host[:, SWEEP_CHANNELS.index(name)]) for name in TABLE_COLUMNS}


def write_sweep(path, sweep: Tensor) -> None:
    """:func:`sweep_table` as an uncompressed feather file (``prototype.loader.read_sweep_table`` reads it back)."""
    from ...prototype.database import _write_feather

    _write_feather(path, sweep_table(sweep))


def batch_from_range_images(range_image: Tensor, extrinsic, inclination, pixel_pose: Optional[Tensor], frame_pose,
                            range_view_config: Mapping[str, Any], padding_mode: str = "constant", pad: bool = True, x_stride: int = 1) -> Dict[str, Tensor]:
    """Range images -> the loader's batch dict in one launch: ``features`` (B, F, H, W') fp32 in ``feature_column_names`` order
    (``intensity`` through tanh, ``loader.py:625-626``), ``cart`` (B, 3, H, W'), ``mask`` (B, 1, H, W') bool, ``num_pts`` (B,) int64.
    ``pad=True``: W' = W + 6 (2650 -> 2656, zeros or ``circular`` wrap-around) -- what the detector eats; ``pad=False``: W' = W, the
    unpadded dict that ``augment_batch`` / ``paste_database`` / ``pad_batch`` take.  Equal bit for bit to :func:`range_image_to_sweep` ->
    :func:`sweep_table` -> ``range_view_from_table(..., "waymo")``."""
    _, ri, ext, inc, pp, inv = _inputs(range_image, extrinsic, inclination, pixel_pose, frame_pose)
    b, h, w, _ = ri.shape
    if int(x_stride) != 1 or int(range_view_config.get("x_stride", 1)) != 1:
        raise L.RvError("batch_from_range_images: x_stride must be 1 (the strided subsampling of the loader is not fused)")
    if int(range_view_config["height"]) != h or int(range_view_config["width"]) != w:
        raise L.RvError(f"range images of {h} x {w}, configured {range_view_config['height']} x {range_view_config['width']}")
    if padding_mode not in ("constant", "circular"):
        raise L.RvError(f"padding_mode {padding_mode!r} (constant or circular)")
    names = list(range_view_config["feature_column_names"])
    unknown = [n for n in names if n not in SWEEP_CHANNELS]
    if unknown:
        raise L.RvError(f"features {unknown} are not columns of a Waymo sweep {SWEEP_CHANNELS}")
    n_pad = _PAD[("waymo", 1)] if pad else 0
    feat_src = (ctypes.c_int32 * len(names))(*[SWEEP_CHANNELS.index(n) for n in names])
    feat_op = (ctypes.c_int32 * len(names))(*[1 if n == "intensity" else 0 for n in names])
    dev = ri.device
    features = torch.empty((b, len(names), h, w + 2 * n_pad), dtype=torch.float32, device=dev)
    cart = torch.empty((b, 3, h, w + 2 * n_pad), dtype=torch.float32, device=dev)
    mask = torch.empty((b, 1, h, w + 2 * n_pad), dtype=torch.uint8, device=dev)
    num_pts = torch.empty(b, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        L.call("rv_waymo_range_image_to_batch", L.ptr(ri), L.ptr(ext), L.ptr(inc), L.ptr(pp), L.ptr(inv), b, h, w,
               len(names), feat_src, feat_op, n_pad, 1 if padding_mode == "circular" else 0, L.ptr(features), L.ptr(cart),
               L.ptr(mask), L.ptr(num_pts), L.stream_ptr())
    return {"features": features, "cart": cart, "mask": mask.bool(), "num_pts": num_pts}


def labels_to_annotations(labels: Mapping[str, Sequence], timestamp_ns: int, log_id: Optional[str] = None):
    """``export_annotations`` / ``build_argo_label`` (``export.py:415-501``) for one frame: ``labels`` maps ``type, center_x, center_y,
    center_z, length, width, height, heading, num_lidar_points_in_box, detection_difficulty_level, id`` to one entry per label.  SIGN (3)
    and UNKNOWN (0) are dropped; heading h -> ``qw = cos(h / 2), qz = sin(h / 2), qx = qy = 0``.  ``track_uuid`` is the label's id itself
    (the reference draws a random uuid per id: the id is the deterministic choice).  Returns an Arrow table with the reference's
    columns (+ ``log_id`` when given) that ``annotations_for_sweep`` and ``evaluate_waymo`` take as it is."""
    import pyarrow as pa

    kind = np.asarray(labels["type"], dtype=np.int64).reshape(-1)
    if kind.size and (kind.min() < 0 or kind.max() >= len(LABEL_TYPES)):
        raise L.RvError(f"label types {sorted(set(kind.tolist()) - set(range(len(LABEL_TYPES))))} are not Waymo label types 0 .. 4")
    keep = np.flatnonzero((kind != LABEL_TYPES.index("SIGN")) & (kind != LABEL_TYPES.index("UNKNOWN")))
    col = lambda name: np.asarray(labels[name], dtype=np.float64).reshape(-1)[keep]  # noqa: E731
    heading = col("heading")
    n = keep.size
    cols = {"timestamp_ns": pa.array(np.full(n, int(timestamp_ns), dtype=np.int64)),
            "track_uuid": pa.array([str(labels["id"][i]) for i in keep], type=pa.string()),
            "category": pa.array([LABEL_TYPES[int(kind[i])] for i in keep], type=pa.string()),
            "length_m": pa.array(col("length")), "width_m": pa.array(col("width")), "height_m": pa.array(col("height")),
            "qw": pa.array(np.cos(heading / 2.0)), "qx": pa.array(np.zeros(n)), "qy": pa.array(np.zeros(n)), "qz": pa.array(np.sin(heading / 2.0)),
            "tx_m": pa.array(col("center_x")), "ty_m": pa.array(col("center_y")), "tz_m": pa.array(col("center_z")),
            "num_interior_pts": pa.array(np.asarray(labels["num_lidar_points_in_box"], dtype=np.int64).reshape(-1)[keep]),
            "difficulty_level": pa.array(np.asarray(labels["detection_difficulty_level"], dtype=np.int64).reshape(-1)[keep])}
    if log_id is not None:
        cols["log_id"] = pa.array([str(log_id)] * n, type=pa.string())
    return pa.table(cols)
