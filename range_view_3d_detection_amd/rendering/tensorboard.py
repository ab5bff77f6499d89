"""The training loop's debug panels (``rendering/tensorboard.py`` of the reference: ``to_logger`` / ``draw_detections``, called from
``nn/arch/detector.py:297-306, 355-364``), built where the tensors already are.  Same names and signatures; bind it with
``from range_view_3d_detection_amd.rendering.tensorboard import to_logger``.

The reference slices sample 0, copies ``cart``, the logits and the aux loss maps to the host, splats the bird's-eye view with an index
store, draws with cv2 and makes one round trip to the GPU for mmcv's ``boxes_iou3d``.  Here every per-pixel step is a kernel of
``csrc/render.hip`` (declared semantics: ``include/rv3d_render.h``) writing blocks of ONE planar uint8 image
``(3, H_total, W_total)`` on the device; ``to_logger`` makes the single device-to-host copy.  A panel is two launches
(``rv_render_plane``: the scalar plane with its minimum and maximum; ``rv_render_colormap``: normalise, look up, mask, store), the
bird's-eye view one for the points and, with boxes, one for the IoU table plus three stream operations for the footprints.  Nothing
synchronises with the host (after the first call on a device, which uploads the colour tables): the detection frame and the
annotations are host tables, filtered and ranked there and uploaded once, through pinned memory.

Differences from the reference, all declared in the header: the footprints follow an integer raster rule (two pixels wide, not
anti-aliased: cv2 is not available), the aux panels carry no text label (there is no cv2 font), and a point or corner that lands on
row or column ``side`` is dropped where the reference's index store would raise.

The module imports neither Lightning, cv2, kornia, mmcv nor matplotlib; the trainer and the logger are recognised by duck typing.
"""

from __future__ import annotations

import ctypes
import math
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _lib as L
from ..math.ops.coding import DETECTION_COLUMNS, _column

COLS = DETECTION_COLUMNS
PLANE_NORM, PLANE_LIKELIHOOD, PLANE_ABS, PLANE_IDENTITY = 0, 1, 2, 3  # RV_PLANE_*
_TABLES = {"GREYS": 0, "TURBO_R": 1, "VIRIDIS": 2}  # RV_CMAP_*
RED, GREEN, BLUE = 1, 2, 4  # channel bits of rv_render_bev_boxes
IOU_GREEN = 0.7

_host_tables: Dict[str, Tensor] = {}
_device_tables: Dict[Tuple[str, torch.device], Tensor] = {}


def _table(name: str) -> Tensor:
    """(3, 256) uint8 host tensor, the reference's layout, copied out of the library (which holds the only copy)."""
    if name not in _host_tables:
        buf = (ctypes.c_uint8 * 768)()
        if L.load().rv_render_colormap_table(_TABLES[name], ctypes.addressof(buf)) != 0:
            raise L.RvError(f"rv_render_colormap_table failed: {L.load().rv_last_error().decode()}")
        _host_tables[name] = torch.frombuffer(bytearray(buf), dtype=torch.uint8).reshape(256, 3).t().contiguous()
    return _host_tables[name]


def __getattr__(name: str):  # GREYS, TURBO_R, VIRIDIS: read from the library on first use
    if name in _TABLES:
        return _table(name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _lut(colormap, device: torch.device) -> Tensor:
    """Device copy (3, 256) u8 of a colour table given by name or as the reference's (3, 256) tensor."""
    if isinstance(colormap, str):
        key = (colormap, device)
        if key not in _device_tables:
            _device_tables[key] = _table(colormap).to(device)
        return _device_tables[key]
    if tuple(colormap.shape) != (3, 256) or colormap.dtype != torch.uint8:
        raise L.RvError(f"colormap: (3, 256) uint8 expected, got {tuple(colormap.shape)} {colormap.dtype}")
    return colormap.to(device).contiguous()


def _require_cuda(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise L.RvError(f"{name} must live on the GPU (no CPU fallback)")


def bev_side(max_side: float, meter_per_px: float) -> int:
    return int(math.ceil(max_side * 2 / meter_per_px))


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _plane(src: Tensor, op: int, plane: Tensor, minmax: Tensor) -> None:
    """``rv_render_plane``: src (C,H,W) fp32 contiguous -> plane (H,W) and its min / max keys (``minmax``: 2 zeroed int32 words)."""
    C, H, W = src.shape
    L.call("rv_render_plane", L.ptr(src), H * W, C, H, W, op, L.ptr(plane), L.ptr(minmax), L.stream_ptr())


def _colormap(plane: Tensor, mask: Optional[Tensor], minmax: Tensor, lut: Tensor, image: Tensor, row0: int, col0: int) -> None:
    H, W = plane.shape
    L.call("rv_render_colormap", L.ptr(plane), L.ptr(mask), H, W, L.ptr(minmax), L.ptr(lut), L.ptr(image), image.shape[1], image.shape[2], row0,
           col0, L.stream_ptr())


def _mask_u8(mask: Optional[Tensor], H: int, W: int) -> Optional[Tensor]:
    return None if mask is None else (mask.detach().reshape(H, W) != 0).to(torch.uint8).contiguous()


def normalize_apply_colormap(img: Tensor, colormap, mask: Optional[Tensor] = None) -> Tensor:
    """``img`` (1,1,H,W) -> (3,H,W) uint8: kornia's ``normalize_min_max``, times 255, truncated, looked up in ``colormap`` (a
    (3,256) uint8 tensor, or the name of one of the library's tables), times ``mask``."""
    assert img.ndim == 4
    _require_cuda(img, "img")
    _, _, H, W = img.shape
    with torch.cuda.device(img.device):
        src = img.detach().float().reshape(1, H, W).contiguous()
        plane = torch.empty((H, W), dtype=torch.float32, device=img.device)
        minmax = torch.zeros(2, dtype=torch.int32, device=img.device)
        out = torch.zeros((3, H, W), dtype=torch.uint8, device=img.device)
        _plane(src, PLANE_IDENTITY, plane, minmax)
        _colormap(plane, _mask_u8(mask, H, W), minmax, _lut(colormap, img.device), out, 0, 0)
    return out


def _bev_points(cart: Tensor, max_side: float, meter_per_px: float, side: int, image: Tensor, row0: int, col0: int) -> None:
    """cart (3, n...) fp32 contiguous."""
    n = cart[0].numel()
    L.call("rv_render_bev_points", L.ptr(cart), n, n, float(max_side), float(meter_per_px), side, L.ptr(image), image.shape[1], image.shape[2],
           row0, col0, L.stream_ptr())


def _bev_boxes(boxes: Tensor, scores: Optional[Tensor], channels: Tensor, max_side: float, meter_per_px: float, side: int, image: Tensor,
               row0: int, col0: int) -> None:
    n = boxes.shape[0]
    if n == 0:
        return
    zbuf = torch.empty((side, side), dtype=torch.int32, device=image.device)  # (cleared by the call)
    L.call("rv_render_bev_boxes", L.ptr(boxes), L.ptr(scores), L.ptr(channels), n, float(max_side), float(meter_per_px), side, L.ptr(zbuf),
           L.ptr(image), image.shape[1], image.shape[2], row0, col0, L.stream_ptr())


def build_bev(xyz: Tensor, max_side: float, meter_per_px: float) -> Tensor:
    """``xyz`` (N,3) -> the (side, side, 3) uint8 bird's-eye view with every point inside set to 255 (a view of a planar image)."""
    _require_cuda(xyz, "xyz")
    side = bev_side(max_side, meter_per_px)
    with torch.cuda.device(xyz.device):
        cart = xyz.detach().float().reshape(-1, 3).t().contiguous()
        image = torch.zeros((3, side, side), dtype=torch.uint8, device=xyz.device)
        _bev_points(cart, max_side, meter_per_px, side, image, 0, 0)
    return image.permute(1, 2, 0)


def world_to_image(xyz: Tensor, max_side: float, meter_per_px: float) -> Tensor:
    """The rows of ``xyz`` (N, >= 2) whose x and y fall inside the view, with x and y replaced by their pixel row and column (floats, as in
    the reference; ``xyz`` itself is left alone).  Plain torch on ``xyz``'s device with the kernels' arithmetic (fp32, a true division);
    not on the panels' path -- the kernels map coordinates themselves -- and the selection by a mask synchronises, as in the reference."""
    const = lambda v: torch.tensor(v, dtype=xyz.dtype, device=xyz.device)  # noqa: E731  (a tensor divisor: no reciprocal multiply)
    u = (xyz[:, :2] + const(max_side)) / const(meter_per_px)
    keep = ((u > 0) & (u < const(max_side / meter_per_px * 2.0))).all(dim=-1)
    pixel = torch.floor(const(max_side * 2.0 / meter_per_px) - u)
    return torch.cat([pixel, xyz[:, 2:]], dim=1)[keep]


def _frame_rows(frame, batch_index: Optional[int], with_score: bool) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """((n,10) fp32 rows in ``COLS`` order, scores or None) of a polars / Arrow frame (or a dict of columns), or of the loader's (M,13) annotation rows
    (box, ``task_id``, ``offset``, ``batch_index``), restricted to one sweep; on the host."""
    if isinstance(frame, (Tensor, np.ndarray)):
        rows = (frame.detach().cpu().numpy() if isinstance(frame, Tensor) else frame).reshape(-1, 13)
        if batch_index is not None:
            rows = rows[rows[:, 12].astype(np.int64) == batch_index]
        return np.ascontiguousarray(rows[:, :10], dtype=np.float32), None
    names = set(frame if isinstance(frame, dict) else frame.column_names if hasattr(frame, "column_names") else frame.columns)
    n = len(_column(frame, COLS[0]))
    rows = np.stack([np.asarray(_column(frame, c), dtype=np.float32) for c in COLS], 1) if n else np.zeros((0, 10), np.float32)
    scores = np.asarray(_column(frame, "score"), dtype=np.float32) if with_score and "score" in names else None
    if batch_index is not None and n:
        keep = np.asarray(_column(frame, "batch_index"), dtype=np.int64) == batch_index
        rows, scores = rows[keep], None if scores is None else scores[keep]
    return rows, scores


def _upload(t: Tensor, device: torch.device) -> Tensor:
    """A host tensor to the device through pinned memory, asynchronously: a pageable copy would make the host wait for the stream."""
    return t.contiguous().pin_memory().to(device, non_blocking=True)


def _boxes_host(rows: np.ndarray) -> Tensor:
    """(n,10) host rows -> (n,7) fp32 HOST boxes [x, y, z, l, w, h, yaw]: yaw = atan2(2 (qw qz + qx qy), 1 - 2 (qy^2 + qz^2)) in
    fp64 from the fp32 quaternion, rounded to fp32 with the box (``evaluation.waymo.boxes_from_rows``)."""
    from ..evaluation.waymo import boxes_from_rows

    return boxes_from_rows(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).reshape(-1, 10))


def draw_on_bev(dts, img: Tensor, color: Tuple[int, int, int] = (0, 255, 0), max_side: float = 50.0, meter_per_px: float = 0.1,
                colors=None) -> Tensor:
    """Draws the footprints of ``dts`` (a frame with the ``COLS`` columns and, optionally, ``score``) on the (side, side, 3) uint8
    device image ``img`` and returns the image.  As in the reference, ``color`` is not used: without ``colors`` (n,3) the boxes are
    blue; a box's colour is scaled by its score."""
    _require_cuda(img, "img")
    side = img.shape[0]
    if tuple(img.shape) != (side, side, 3) or side != bev_side(max_side, meter_per_px):
        raise L.RvError(f"draw_on_bev: a ({bev_side(max_side, meter_per_px)},) * 2 + (3,) image expected, got {tuple(img.shape)}")
    rows, scores = _frame_rows(dts, None, True)
    chan = np.full(len(rows), BLUE, np.uint8) if colors is None else \
        ((np.asarray(colors).reshape(-1, 3) != 0) * np.asarray([RED, GREEN, BLUE])).sum(1).astype(np.uint8)
    with torch.cuda.device(img.device):
        planar = img.permute(2, 0, 1).contiguous()
        _bev_boxes(_upload(_boxes_host(rows), img.device), None if scores is None else _upload(torch.from_numpy(scores), img.device),
                   _upload(torch.from_numpy(chan), img.device), max_side, meter_per_px, side, planar, 0, 0)
    return planar.permute(1, 2, 0)


def boxes_iou3d(boxes_a: Tensor, boxes_b: Tensor) -> Tensor:
    """``rv_boxes_iou3d``: (n,7) x (m,7) rows [x, y, z, dx, dy, dz, yaw], z the centre -> (n,m) fp32."""
    a, b = boxes_a.detach().float().contiguous(), boxes_b.detach().float().contiguous()
    out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    L.call("rv_boxes_iou3d", L.ptr(a), a.shape[0], L.ptr(b), b.shape[0], L.ptr(out), L.stream_ptr())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# draw_detections
# ---------------------------------------------------------------------------------------------------------------------------------
def _panel_sources(network_outputs: Dict, b: int) -> List[Tuple[str, Tensor, int, str, Tensor]]:
    """The panels in the reference's order (tensorboard.py:272-425): (kind, (C,H,W) fp32 source, plane op, colour table, (1,H,W)
    mask) -- per level of the head: for stride 1 one likelihood panel per integer task key and the aux panels, the range panel, one
    likelihood panel per task (stride 1 shows it twice)."""
    panels = []
    for stride, level in network_outputs["head"].items():
        mask = level["mask"][b]
        likelihoods = [("likelihood", out["logits"][b], PLANE_LIKELIHOOD, "VIRIDIS", mask) for t, out in level.items() if isinstance(t, int)]
        if stride == 1:
            panels += likelihoods
            if "aux" in network_outputs:
                for t, entries in network_outputs["aux"][stride].items():
                    if isinstance(t, int):
                        panels += [("aux", v[b][ch:ch + 1], PLANE_ABS, "VIRIDIS", mask) for v in entries.values() for ch in range(v.shape[1])]
        panels.append(("range", level["cart"][b], PLANE_NORM, "TURBO_R", mask))
        panels += likelihoods
    return panels


def compose(sizes: Sequence[Tuple[str, int, int]], side: int) -> Tuple[int, int, List[Tuple[int, int]], Tuple[int, int]]:
    """``sizes``: (kind, H, W) per panel in order -> (H_total, W_total, (row0, col0) of every panel, (row0, col0) of the bird's-eye
    view).  The reference's padding: SW starts as the view's side; a panel with W < SW is padded to SW with left = (SW - W) // 2 and the
    rest on the right; at a level's range panel with W >= SW the VIEW is padded to W by the same rule and SW becomes W."""
    sw, bev_col, origins, widths, row = side, 0, [], [], 0
    for kind, h, w in sizes:
        if w < sw:
            origins.append((row, (sw - w) // 2))
            widths.append(sw)
        else:
            origins.append((row, 0))
            widths.append(w)
            if kind == "range":
                bev_col += (w - sw) // 2
                sw = w
        row += h
    if any(wd != sw for wd in widths):  # (torch.cat raises in the reference)
        raise L.RvError(f"the panels do not stack: widths {sorted(set(widths))} against the bird's-eye view's {sw}")
    return row + side, sw, origins, (row, bev_col)


def _draw(dts, data: Dict[str, Any], network_outputs: Dict, max_num_dts: int, max_side: float, meter_per_px: float,
          record: Optional[Dict[str, Any]] = None) -> Tensor:
    batch_index = 0
    head = network_outputs["head"]
    if 1 not in head:
        raise L.RvError("draw_detections: the bird's-eye view is built from the stride-1 level, which network_outputs['head'] lacks")
    dev = head[1]["cart"].device
    _require_cuda(head[1]["cart"], "network_outputs['head'][1]['cart']")
    side = bev_side(max_side, meter_per_px)

    # host tables: the sample's annotations, and its max_num_dts best detections in descending score (ties: frame order)
    ann_rows, _ = _frame_rows(data["annotations"], batch_index, False)
    dt_rows, dt_scores = _frame_rows(dts, batch_index, True)
    if dt_scores is None:
        raise L.RvError("draw_detections: the detection frame has no score column")
    top = np.argsort(-dt_scores, kind="stable")[:max(int(max_num_dts), 0)]
    dt_rows, dt_scores = dt_rows[top], dt_scores[top]
    draw_dts = len(dt_rows) > 0 and len(ann_rows) > 0

    with torch.cuda.device(dev):
        sources = _panel_sources(network_outputs, batch_index)
        H_total, W_total, origins, (bev_row, bev_col) = compose([(k, s.shape[-2], s.shape[-1]) for k, s, _, _, _ in sources], side)
        image = torch.zeros((3, H_total, W_total), dtype=torch.uint8, device=dev)
        minmax = torch.zeros((max(len(sources), 1), 2), dtype=torch.int32, device=dev)
        planes = []
        for i, ((kind, src, op, table, mask), (row0, col0)) in enumerate(zip(sources, origins)):
            _require_cuda(src, f"the source of the {kind} panel")
            src = src.detach().float().contiguous()
            H, W = src.shape[-2:]
            plane = torch.empty((H, W), dtype=torch.float32, device=dev)
            _plane(src, op, plane, minmax[i])
            _colormap(plane, _mask_u8(mask, H, W), minmax[i], _lut(table, dev), image, row0, col0)
            planes.append(plane)

        cart = head[1]["cart"][batch_index].detach().float().contiguous()
        _bev_points(cart, max_side, meter_per_px, side, image, bev_row, bev_col)
        iou = None
        if len(ann_rows) > 0:
            # one upload: the annotations' boxes with score 1, then the detections' with theirs, (n, 8)
            n_ann = len(ann_rows)
            table = torch.cat([_boxes_host(ann_rows), torch.ones(n_ann, 1)], 1)
            if draw_dts:
                table = torch.cat([table, torch.cat([_boxes_host(dt_rows), torch.from_numpy(dt_scores)[:, None]], 1)])
            table = _upload(table, dev)
            boxes, scores = table[:, :7].contiguous(), table[:, 7].contiguous()
            channels = torch.full((n_ann,), BLUE, dtype=torch.uint8, device=dev)
            if draw_dts:
                iou = boxes_iou3d(boxes[n_ann:], boxes[:n_ann])
                colour = torch.where(iou.max(dim=-1).values >= IOU_GREEN, GREEN, RED).to(torch.uint8)
                channels = torch.cat([channels, colour])
            _bev_boxes(boxes, scores, channels, max_side, meter_per_px, side, image, bev_row, bev_col)
    if record is not None:
        record.update(kinds=[k for k, *_ in sources], tables=[t for _, _, _, t, _ in sources], masks=[m for *_, m in sources], planes=planes,
                      origins=origins, bev_origin=(bev_row, bev_col), side=side, iou=iou, annotations=ann_rows, detections=dt_rows,
                      scores=dt_scores)
    return image


def draw_detections(dts, uuids, data: Dict[str, Any], network_outputs: Dict, max_num_dts: int = 500, max_side: float = 75.0,
                    meter_per_px: float = 0.15) -> Tensor:
    """The (3, H_total, W_total) uint8 image of sample 0, a DEVICE tensor: per level of ``network_outputs["head"]`` the panels of
    ``_panel_sources``, then the bird's-eye view with the stride-1 points, the sample's annotations in blue and -- only with at least
    one detection AND one annotation -- its ``max_num_dts`` best detections in descending score, green where their best 3-D IoU with
    an annotation is >= 0.7 and red otherwise, scaled by the score.  ``dts``: what ``build_dataframe`` returns (an Arrow table) or a
    polars frame; ``data["annotations"]``: a polars / Arrow frame or the loader's (M,13) rows.  ``uuids`` is not used (as in the
    reference)."""
    return _draw(dts, data, network_outputs, max_num_dts, max_side, meter_per_px)


# ---------------------------------------------------------------------------------------------------------------------------------
# loggers
# ---------------------------------------------------------------------------------------------------------------------------------
def _stage(trainer) -> str:
    stage = getattr(getattr(trainer, "state", None), "stage", None)
    return str(getattr(stage, "value", stage))


def _is_rank_zero(trainer) -> bool:
    rank = getattr(trainer, "global_rank", None)
    if rank is None:
        rank = next((int(os.environ[k]) for k in ("RANK", "LOCAL_RANK", "SLURM_PROCID") if k in os.environ), 0)
    return int(rank) == 0


def to_logger(dts, uuids, data: Dict[str, Any], network_outputs: Dict, tasks_cfg, trainer, debug: bool, batch_index: int,
              max_num_dts: int = 100, max_side: float = 75.0, meter_per_px: float = 0.15) -> None:
    """Rank zero only, and nothing during Lightning's sanity check: draws the panels on the device, copies the image to the host
    (the single device-to-host copy) and hands it to the trainer's logger under ``<log_id>-<timestamp_ns>`` of ``batch_index``."""
    if not _is_rank_zero(trainer):
        return
    if _stage(trainer) == "sanity_check" or getattr(trainer, "sanity_checking", False):
        return
    img = draw_detections(dts=dts, uuids=uuids, data=data, network_outputs=network_outputs, max_num_dts=max_num_dts, max_side=max_side,
                          meter_per_px=meter_per_px)
    row = next(i for i, b in enumerate(_column(uuids, "batch_index")) if int(b) == batch_index)
    prefix = f"{_column(uuids, 'log_id')[row]}-{_column(uuids, 'timestamp_ns')[row]}"
    log_image(name=prefix, img=img.cpu().numpy(), trainer=trainer)


def log_image(name: str, img, trainer) -> None:
    """``img``: the (3,H,W) uint8 image on the host.  A logger with ``log_image`` (``WandbLogger``) gets
    ``log_image(stage, [HWC image], caption=[name])``; one whose ``experiment`` has ``add_image`` (``TensorBoardLogger``) gets
    ``add_image(f"{stage}/{name}", CHW image, global_step=trainer.global_step)``; any other logger, or none, gets nothing."""
    logger = getattr(trainer, "logger", None)
    if logger is None:
        return
    img = np.asarray(img.cpu() if isinstance(img, Tensor) else img)
    stage = _stage(trainer)
    if callable(getattr(logger, "log_image", None)):
        logger.log_image(f"{stage}", [np.ascontiguousarray(img.transpose(1, 2, 0))], caption=[name])
    elif callable(getattr(getattr(logger, "experiment", None), "add_image", None)):
        logger.experiment.add_image(f"{stage}/{name}", img, global_step=trainer.global_step)
