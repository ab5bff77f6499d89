"""``detectron2.layers.nms.nms_rotated`` -- the function the reference binds for ``nms_mode: HARD``, on ``librv3d_hip.so``.

The reference calls (``src/torchbox3d/math/ops/nms.py:6,39-44``)::

    from detectron2.layers.nms import nms_rotated
    input[:, -1] = -input[:, -1].rad2deg()
    keep_ij = nms_rotated(boxes=input.type(torch.float32), scores=scores_ij.type(torch.float32),
                          iou_threshold=torch.as_tensor(iou_threshold))

with detectron2's contract: ``boxes`` (N,5) = ``(cx, cy, w, h, angle in degrees)``, ``scores`` (N,), both unsorted;
``iou_threshold`` a float (or a 0-d tensor, as the reference passes it); returns the int64 indices of the kept boxes, on the
boxes' device, in descending score order.  Bind it with ``from range_view_3d_detection_amd.compat.detectron2_nms import
nms_rotated`` and the reference's ``hard_multiclass_nms`` (``nms.py:10-61``) runs unchanged.

The arithmetic is ``rv_nms_rotated`` (csrc/nms.hip; declared semantics in include/rv3d.h -- detectron2 is not part of the
reference tree, parity unpinned at the last bit of the IoU): boxes are visited in descending score order, equal scores in
ascending index order (a stable sort on the device); a kept box suppresses the later boxes whose rotated IoU with it is
strictly greater than ``iou_threshold``.  detectron2's ``angle`` runs counter-clockwise in image coordinates (y pointing down: the
width axis lies at ``(cos a, -sin a)``), which is why the reference negates the yaw; the rectangle handed to the kernel is
``[cx - w/2, cy - h/2, cx + w/2, cy + h/2, -angle * pi / 180]``.  No CPU fallback: host tensors raise.
"""

from __future__ import annotations

import math
from typing import Union

import torch
from torch import Tensor

from range_view_3d_detection_amd import _lib as L


def nms_rotated(boxes: Tensor, scores: Tensor, iou_threshold: Union[float, Tensor]) -> Tensor:
    for name, t in (("boxes", boxes), ("scores", scores)):
        if not t.is_cuda:
            raise L.RvError(f"nms_rotated: {name} must live on the GPU (no CPU fallback)")
    if boxes.dim() != 2 or boxes.shape[1] != 5 or scores.shape != (boxes.shape[0],):
        raise L.RvError(f"nms_rotated: boxes (N,5) and scores (N,) expected, got {tuple(boxes.shape)} and {tuple(scores.shape)}")
    if boxes.shape[0] == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    from range_view_3d_detection_amd.math.ops.nms import nms_rotated_sorted

    with torch.cuda.device(boxes.device):
        order = scores.float().sort(dim=0, descending=True, stable=True).indices
        b = boxes.float()[order]
        half = b[:, 2:4] / 2
        rect = torch.cat([b[:, :2] - half, b[:, :2] + half, b[:, 4:5] * (-math.pi / 180.0)], dim=1)
        return order[nms_rotated_sorted(rect, float(iou_threshold))]
