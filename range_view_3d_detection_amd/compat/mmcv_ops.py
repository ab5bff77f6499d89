"""``mmcv.ops.boxes_iou3d`` and ``mmcv.ops.box_iou_rotated`` -- the two mmcv CUDA ops the reference imports, on ``librv3d_hip.so``.

The reference binds them by name::

    from mmcv.ops import boxes_iou3d        # rendering/tensorboard.py:14, the colour of a detection in the debug panel
    from mmcv.ops import box_iou_rotated    # the loader's collision test, the BEV affinity of soft assignment

Bind ``from range_view_3d_detection_amd.compat.mmcv_ops import boxes_iou3d, box_iou_rotated`` instead.  mmcv is
not part of the reference tree, so the last bit of either IoU is not pinned; the semantics are DECLARED in ``include/rv3d_render.h``.

``boxes_iou3d(boxes_a, boxes_b)``: (n,7) x (m,7) rows ``[x, y, z, dx, dy, dz, yaw]`` with ``z`` the box CENTRE (what
``tensorboard.py:296-314`` passes) -> (n,m) fp32 3-D IoU, ``rv_boxes_iou3d``: the arithmetic of the Waymo evaluator's 3-D column,
bit for bit, with no limit on the row counts.

``box_iou_rotated(bboxes1, bboxes2, mode="iou", aligned=False, clockwise=True)``: boxes ``(cx, cy, w, h, angle in radians)``.
ANGLE CONVENTION (worked out in ``tests/golden/make_golden_database.py``): mmcv's box has its first extent along ``(cos a, sin a)``
in the coordinates it is given -- "clockwise" refers to image coordinates, y pointing down -- so the rectangle handed to the kernel is
``[cx - w/2, cy - h/2, cx + w/2, cy + h/2, ry = +a]``.  Dense: ``rv_rotated_iou`` (n,m).  ``aligned=True``: (n,) of the pairs
``(bboxes1[k], bboxes2[k])``, computed per pair by ``rv_rotated_iou_pairs`` (no n x n table), bit-equal to the dense diagonal.
``mode="iof"`` and ``clockwise=False`` raise ``NotImplementedError``.  No CPU fallback: host tensors raise.
"""

from __future__ import annotations

import torch
from torch import Tensor

from range_view_3d_detection_amd import _lib as L


def _require(t: Tensor, name: str, width: int, who: str) -> Tensor:
    if not t.is_cuda:
        raise L.RvError(f"{who}: {name} must live on the GPU (no CPU fallback)")
    if t.dim() != 2 or t.shape[1] != width:
        raise L.RvError(f"{who}: {name} (N,{width}) expected, got {tuple(t.shape)}")
    return t.detach().float().contiguous()


def boxes_iou3d(boxes_a: Tensor, boxes_b: Tensor) -> Tensor:
    a, b = _require(boxes_a, "boxes_a", 7, "boxes_iou3d"), _require(boxes_b, "boxes_b", 7, "boxes_iou3d")
    with torch.cuda.device(a.device):
        out = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
        L.call("rv_boxes_iou3d", L.ptr(a), a.shape[0], L.ptr(b), b.shape[0], L.ptr(out), L.stream_ptr())
    return out


def _rect(b: Tensor) -> Tensor:
    half = b[:, 2:4] / 2
    return torch.cat([b[:, :2] - half, b[:, :2] + half, b[:, 4:5]], dim=1).contiguous()


def box_iou_rotated(bboxes1: Tensor, bboxes2: Tensor, mode: str = "iou", aligned: bool = False, clockwise: bool = True) -> Tensor:
    if mode != "iou":
        raise NotImplementedError(f"box_iou_rotated: mode {mode!r} (only 'iou')")
    if not clockwise:
        raise NotImplementedError("box_iou_rotated: clockwise=False")
    a, b = _require(bboxes1, "bboxes1", 5, "box_iou_rotated"), _require(bboxes2, "bboxes2", 5, "box_iou_rotated")
    n, m = a.shape[0], b.shape[0]
    if aligned and n != m:
        raise L.RvError(f"box_iou_rotated: aligned=True takes as many boxes on either side, got {n} and {m}")
    with torch.cuda.device(a.device):
        ra, rb = _rect(a), _rect(b)
        if aligned:
            out = torch.zeros(n, dtype=torch.float32, device=a.device)
            L.call("rv_rotated_iou_pairs", L.ptr(ra), L.ptr(rb), n, L.ptr(out), L.stream_ptr())
        else:
            out = torch.zeros((n, m), dtype=torch.float32, device=a.device)
            L.call("rv_rotated_iou", L.ptr(ra), n, L.ptr(rb), m, L.ptr(out), L.stream_ptr())
    return out
