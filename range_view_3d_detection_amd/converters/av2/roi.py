"""AV2 region of interest (ROI) on the device: the map raster of every log in one atlas, per-point and per-box flags.

Replaces the two places where the reference goes through av2's CPU map API -- the converter's ``is_within_roi`` column
(``converters/av2/export.py:91-97``: ``city_SE3_egovehicle.transform_from`` + ``avm.get_raster_layer_points_boolean(city_xyz, ROI)``) and
the evaluation filter ``eval_only_roi_instances`` (``datasets/__init__.py:27-30``).  Both are one operation: ego frame -> city frame ->
the log's ROI raster.  av2 is not part of the reference tree: the semantics are DECLARED in ``include/rv3d.h`` and not
pinned against av2's binaries.  Arrays go in; reading the map JSON and the pose feather files stays with the caller.

* :class:`RoiAtlas` -- the rasters of any number of logs in one device buffer.  ``RoiAtlas.from_rasters`` takes av2's own
  ``raster_roi_layer.array`` and the ``(s, tx, ty)`` of its ``array_Sim2_city`` (R = I), so a user who holds av2 looks up av2's raster
  bit for bit; :func:`build_roi_raster` builds a layer from drivable-area polygons for a user who does not;
* :func:`roi_points` -- ``rv_roi_points``: the ``is_within_roi`` flag of every lidar return of a batch of sweeps, i.e.
  ``features[:, 5]`` of ``converters.av2.utils.build_range_view``;
* :func:`roi_boxes` -- ``rv_roi_boxes``: a box is inside iff any of its 8 vertices is (``evaluation.DetectionEvaluator`` uses it);
* :func:`rasterize_polygons`, :func:`build_roi_raster` -- ``rv_roi_rasterize``: even-odd fill at the pixel centres, then a dilation.

No CPU fallback.
"""

from __future__ import annotations

import ctypes
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from ... import _lib as L
from ...engine import _require_cuda

_LAYER_DTYPE = np.dtype([("offset", "<i8"), ("height", "<i4"), ("width", "<i4"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8")])  # rvRoiLayer


class RoiAtlas:
    """The ROI rasters of several logs: ``raster`` (bytes,) uint8, ``layers`` the ``rvRoiLayer`` table as (n_layers * 40,) uint8, both on
    ``device``; ``log_ids[k]`` names layer k."""

    def __init__(self, log_ids: Sequence[str], raster: Tensor, layers: Tensor, records: np.ndarray) -> None:
        self.log_ids: Tuple[str, ...] = tuple(str(l) for l in log_ids)
        self.raster, self.layers, self.records = raster, layers, records
        self._index = {l: k for k, l in enumerate(self.log_ids)}

    @classmethod
    def from_rasters(cls, log_ids: Sequence[str], arrays: Sequence[Any], sims: Sequence[Tuple[float, float, float]]) -> "RoiAtlas":
        """``arrays[k]`` (height, width) bool / uint8: cell ``[v, u]`` of log ``log_ids[k]``; ``sims[k]`` = ``(s, tx, ty)``: raster
        coordinates are ``((x + tx) * s, (y + ty) * s)`` of the city point.  The atlas is built on the host (one buffer, one upload with
        :meth:`to`); the table is checked against the buffer size before anything can be looked up."""
        log_ids = [str(l) for l in log_ids]
        if not (len(log_ids) == len(arrays) == len(sims)):
            raise L.RvError(f"{len(log_ids)} log ids, {len(arrays)} rasters, {len(sims)} transforms")
        if len(set(log_ids)) != len(log_ids):
            raise L.RvError("RoiAtlas: a log id appears twice")
        records, flat, offset = np.zeros(len(log_ids), dtype=_LAYER_DTYPE), [], 0
        for k, (arr, sim) in enumerate(zip(arrays, sims)):
            a = np.asarray(arr.detach().cpu().numpy() if isinstance(arr, Tensor) else arr)
            if a.ndim != 2 or a.size == 0:
                raise L.RvError(f"raster of log {log_ids[k]} has shape {a.shape}, expected (height, width)")
            s, tx, ty = (float(v) for v in sim)
            records[k] = (offset, a.shape[0], a.shape[1], s, tx, ty)
            flat.append(np.ascontiguousarray(a != 0).astype(np.uint8).reshape(-1))
            offset += a.size
        raster = np.concatenate(flat) if flat else np.zeros(0, np.uint8)
        if len(log_ids):
            L.call("rv_roi_atlas_check", ctypes.c_void_p(records.ctypes.data), len(log_ids), raster.size)
        return cls(log_ids, torch.from_numpy(raster), torch.from_numpy(records.view(np.uint8).copy()), records)

    @property
    def device(self) -> torch.device:
        return self.raster.device

    @property
    def n_layers(self) -> int:
        return len(self.log_ids)

    def to(self, device: Any) -> "RoiAtlas":
        dev = torch.device(device)
        return self if dev == self.device else RoiAtlas(self.log_ids, self.raster.to(dev), self.layers.to(dev), self.records)

    def layer_of(self, log_id: str) -> int:
        """Index of the log's layer (what ``layer_index`` holds); an unknown log raises."""
        k = self._index.get(str(log_id))
        if k is None:
            raise L.RvError(f"the ROI atlas holds no raster for log {log_id!r} ({self.n_layers} logs)")
        return k

    def layer(self, k: int) -> Tuple[np.ndarray, Tuple[float, float, float]]:
        """Host copy of layer k: ``(array (height, width) uint8, (s, tx, ty))``."""
        r = self.records[k]
        n = int(r["height"]) * int(r["width"])
        arr = self.raster[int(r["offset"]):int(r["offset"]) + n].cpu().numpy().reshape(int(r["height"]), int(r["width"]))
        return arr, (float(r["s"]), float(r["tx"]), float(r["ty"]))


def _sweep_table(layer_index, city_SE3_ego, atlas: RoiAtlas, dev) -> Tuple[Tensor, Tensor, RoiAtlas]:
    if not isinstance(atlas, RoiAtlas):
        raise L.RvError(f"atlas is a {type(atlas).__name__}, expected a RoiAtlas")
    layer = torch.as_tensor(layer_index).to(dev).reshape(-1).to(torch.int32).contiguous()
    pose = torch.as_tensor(city_SE3_ego).to(dev).to(torch.float64)
    if pose.dim() == 3 and tuple(pose.shape[1:]) == (4, 4):
        pose = pose[:, :3, :]
    pose = pose.reshape(-1, 12).contiguous()
    if layer.shape[0] < 1 or pose.shape[0] != layer.shape[0]:
        raise L.RvError(f"{layer.shape[0]} layer indices, {pose.shape[0]} poses (one of each per sweep, at least one sweep)")
    return layer, pose, atlas.to(dev)


def _stray_counter(stray: Optional[Tensor], dev) -> Tensor:
    if stray is None:
        return torch.zeros((), dtype=torch.int64, device=dev)
    if stray.dtype != torch.int64 or stray.device != dev or stray.numel() != 1:
        raise L.RvError("stray must be one int64 on the device of the rows")
    return stray


def _raise_on_stray(count: Tensor, what: str) -> None:
    if int(count) != 0:
        raise L.RvError(f"{int(count)} {what} belong to no sweep")


def roi_points(xyz: Tensor, sweep_offsets, layer_index, city_SE3_ego, atlas: RoiAtlas, stray: Optional[Tensor] = None) -> Tensor:
    """``xyz`` (N, 3) fp32 or fp64 ego-frame points of B sweeps laid end to end, ``sweep_offsets`` (B + 1,) int64 (CSR), ``layer_index``
    (B,) (:meth:`RoiAtlas.layer_of`; a value that names no layer flags nothing), ``city_SE3_ego`` (B, 3, 4) -> (N,) uint8
    ``is_within_roi``.  One launch; asynchronous when ``stray`` (one int64 on the device, accumulated: rows outside every sweep) is
    given; without it the count is read back and a non-zero count raises."""
    _require_cuda(xyz, "xyz")
    dev = xyz.device
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise L.RvError(f"xyz has shape {tuple(xyz.shape)}, expected (N, 3)")
    pts = (xyz if xyz.dtype == torch.float64 else xyz.float()).contiguous()
    layer, pose, atlas = _sweep_table(layer_index, city_SE3_ego, atlas, dev)
    off = torch.as_tensor(sweep_offsets).to(dev).reshape(-1).to(torch.int64).contiguous()
    if off.shape[0] != layer.shape[0] + 1:
        raise L.RvError(f"{off.shape[0]} sweep offsets for {layer.shape[0]} sweeps (one more than sweeps)")
    out = torch.empty(pts.shape[0], dtype=torch.uint8, device=dev)
    count = _stray_counter(stray, dev)
    with torch.cuda.device(dev):
        L.call("rv_roi_points", L.ptr(pts), 1 if pts.dtype == torch.float64 else 0, pts.shape[0], L.ptr(off), layer.shape[0],
               L.ptr(layer), L.ptr(pose), L.ptr(atlas.raster), atlas.raster.numel(), L.ptr(atlas.layers), atlas.n_layers, L.ptr(out),
               L.ptr(count), L.stream_ptr())
    if stray is None:
        _raise_on_stray(count, "points")
    return out


def roi_boxes(boxes: Tensor, batch_index: Tensor, layer_index, city_SE3_ego, atlas: RoiAtlas, stray: Optional[Tensor] = None) -> Tensor:
    """``boxes`` (N, 10) rows in ``DETECTION_COLUMNS`` order (ego frame), ``batch_index`` (N,) the sweep of each -> (N,) uint8: 1 iff any
    of the box's 8 vertices lies in the ROI of its sweep's log.  ``stray`` as for :func:`roi_points` (a ``batch_index`` outside [0, B))."""
    _require_cuda(boxes, "boxes")
    dev = boxes.device
    rows = boxes.detach().float().reshape(-1, 10).contiguous()
    bidx = batch_index.detach().to(dev).reshape(-1).to(torch.int64).contiguous()
    if bidx.shape[0] != rows.shape[0]:
        raise L.RvError(f"{rows.shape[0]} boxes, {bidx.shape[0]} batch indices")
    layer, pose, atlas = _sweep_table(layer_index, city_SE3_ego, atlas, dev)
    out = torch.empty(rows.shape[0], dtype=torch.uint8, device=dev)
    count = _stray_counter(stray, dev)
    with torch.cuda.device(dev):
        L.call("rv_roi_boxes", L.ptr(rows), L.ptr(bidx), rows.shape[0], layer.shape[0], L.ptr(layer), L.ptr(pose), L.ptr(atlas.raster),
               atlas.raster.numel(), L.ptr(atlas.layers), atlas.n_layers, L.ptr(out), L.ptr(count), L.stream_ptr())
    if stray is None:
        _raise_on_stray(count, "boxes")
    return out


def rasterize_polygons(vertices: Tensor, polygon_offsets: Tensor, s: float, tx: float, ty: float, height: int, width: int,
                       radius_px: float) -> Tuple[Tensor, Tensor]:
    """``rv_roi_rasterize``: ``vertices`` (V, 2) fp64 city frame, ``polygon_offsets`` (P + 1,) int64 (polygon p = the closed ring of its
    vertices) -> (``drivable``, ``roi``), both (height, width) uint8 on the device: the even-odd fill at the pixel centres and its
    dilation by ``radius_px`` pixels.  Asynchronous."""
    _require_cuda(vertices, "vertices")
    dev = vertices.device
    verts = vertices.to(torch.float64).reshape(-1, 2).contiguous()
    off = polygon_offsets.to(dev).reshape(-1).to(torch.int64).contiguous()
    if off.shape[0] < 1:
        raise L.RvError("polygon_offsets is empty (P + 1 entries)")
    height, width = int(height), int(width)
    drivable = torch.empty((height, width), dtype=torch.uint8, device=dev)
    roi = torch.empty((height, width), dtype=torch.uint8, device=dev)
    n_poly = off.shape[0] - 1
    ws_bytes = L.load().rv_roi_rasterize_workspace_bytes(n_poly, height, width)
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        L.call("rv_roi_rasterize", L.ptr(verts), L.ptr(off), verts.shape[0], n_poly, s, tx, ty, height,
               width, radius_px, L.ptr(ws), L.ptr(drivable), L.ptr(roi), L.stream_ptr())
    return drivable, roi


def build_roi_raster(polygons: Sequence[Any], resolution_m: float, dilation_m: float, margin_m: Optional[float] = None,
                     device: Any = "cuda") -> Tuple[np.ndarray, Tuple[float, float, float]]:
    """A ROI layer from a log's drivable-area polygons (city frame, (n, 2) or (n, 3) each; z is ignored): the drivable area filled at
    ``resolution_m`` metres per pixel and dilated by ``dilation_m`` metres.  The raster spans the polygons' bounding box grown by
    ``margin_m`` (default: ``dilation_m``, so that the dilation is not cut off), with a whole-metre origin: ``tx = -floor(min x -
    margin)``.  Returns ``(array (height, width) uint8, (s, tx, ty))`` -- what :meth:`RoiAtlas.from_rasters` takes.  The dataset's own
    resolution and dilation are the caller's to supply: they are not part of this tree."""
    res, dil = float(resolution_m), float(dilation_m)
    if not (res > 0 and np.isfinite(res) and dil >= 0 and np.isfinite(dil)):
        raise L.RvError(f"resolution_m = {resolution_m}, dilation_m = {dilation_m}")
    margin = dil if margin_m is None else float(margin_m)
    rings: List[np.ndarray] = [np.asarray(p, dtype=np.float64).reshape(len(p), -1)[:, :2] for p in polygons]
    if not rings or sum(len(r) for r in rings) == 0:
        raise L.RvError("build_roi_raster: no polygon vertices")
    verts = np.ascontiguousarray(np.concatenate(rings))
    if not np.isfinite(verts).all():
        raise L.RvError("build_roi_raster: a polygon vertex is not finite")
    s = 1.0 / res
    lo, hi = np.floor(verts.min(0) - margin), verts.max(0) + margin
    tx, ty = float(-lo[0]), float(-lo[1])
    width, height = int(np.ceil((hi[0] + tx) * s)) + 1, int(np.ceil((hi[1] + ty) * s)) + 1
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise L.RvError(f"build_roi_raster on {dev}: the raster kernels only run on an MI355X (no CPU fallback)")
    _, roi = rasterize_polygons(torch.from_numpy(verts).to(dev), torch.from_numpy(offsets).to(dev), s, tx, ty, height, width, dil * s)
    return roi.cpu().numpy(), (s, tx, ty)
