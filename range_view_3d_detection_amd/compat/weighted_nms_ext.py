"""``weighted_nms_ext`` -- the op-level FFI the reference binds for weighted NMS, on ``librv3d_hip.so``.

The reference calls (``/root/reference/src/torchbox3d/math/ops/nms.py:161-170``)::

    num_out = weighted_nms_ext.wnms_gpu(boxes, data2merge_score, output, keep, count,
                                        nms_threshold, merge_thresh, boxes.device.index)

with the TorchEx contract: inputs sorted by score descending; ``boxes`` f32 (N,5) [x1,y1,x2,y2,ry] on the
device; ``data2merge_score`` f32 (N,C+1) on the device, last column = score; ``output`` f32 (N,C+1) zero-initialised by the
caller, rows ``[0, num_out)`` filled in place; ``keep`` **int64 on the HOST** (N,), entries ``[0, num_out)`` filled with the
indices (into the sorted order) of the kept boxes; ``count`` int64 (N,) on the device, members merged into each kept box;
returns ``num_out`` as a Python int (synchronous); no stream argument -- the current stream of ``device_index``.
Post-conditions the caller asserts (``nms.py:173-174``): ``output[num_out:] == 0`` and ``count[:num_out] > 0``.

The arithmetic is ``rv_wnms`` (csrc/nms.hip; declared semantics in oracle/nms.py -- the TorchEx source is not part of the
reference tree, parity unpinned).  No CPU fallback: host tensors for boxes/data raise.

``wnms_gpu`` keeps TorchEx's fixed signature, so the declaration's free choices (``WnmsSemantics``) cannot be an argument:
``with weighted_nms_ext.semantics(s):`` governs the calls inside the block.  That is module-level state, acceptable only here -- in a
module that imitates a third-party one; everywhere else the setting is a per-call argument.  Outside any block the declaration applies.
"""

from __future__ import annotations

import torch
from torch import Tensor

from range_view_3d_detection_amd import _lib as L
from range_view_3d_detection_amd.math.ops.nms import WnmsSemantics, wnms_sorted

_SEMANTICS = None  # the setting of the innermost `semantics(...)` block; None: the declaration


class semantics:
    """``with semantics(WnmsSemantics(...)):`` -- ``wnms_gpu`` inside the block computes under that setting."""

    def __init__(self, setting: WnmsSemantics) -> None:
        if not isinstance(setting, WnmsSemantics):
            raise L.RvError(f"semantics() takes a WnmsSemantics, got {type(setting).__name__}")
        self.setting = setting

    def __enter__(self):
        global _SEMANTICS
        self.old, _SEMANTICS = _SEMANTICS, self.setting
        return self

    def __exit__(self, *exc):
        global _SEMANTICS
        _SEMANTICS = self.old


def wnms_gpu(boxes: Tensor, data2merge_score: Tensor, output: Tensor, keep: Tensor, count: Tensor, nms_thresh: float,
             merge_thresh: float, device_index: int) -> int:
    for name, t in (("boxes", boxes), ("data2merge_score", data2merge_score), ("output", output), ("count", count)):
        if not t.is_cuda:
            raise L.RvError(f"wnms_gpu: {name} must live on the GPU (no CPU fallback)")
        if not t.is_contiguous():
            raise L.RvError(f"wnms_gpu: {name} must be contiguous")
    if boxes.dtype != torch.float32 or data2merge_score.dtype != torch.float32 or output.dtype != torch.float32:
        raise L.RvError("wnms_gpu: boxes / data2merge_score / output must be float32")
    if count.dtype != torch.int64 or keep.dtype != torch.int64 or keep.is_cuda:
        raise L.RvError("wnms_gpu: keep must be a host int64 tensor, count a device int64 tensor")
    n, d = data2merge_score.shape
    if boxes.shape != (n, 5) or output.shape != (n, d) or keep.numel() < n or count.numel() < n:
        raise L.RvError("wnms_gpu: shape mismatch")
    if device_index is not None and boxes.device.index != device_index:
        raise L.RvError(f"wnms_gpu: tensors are on cuda:{boxes.device.index}, device_index says {device_index}")
    if n == 0:
        return 0
    with torch.cuda.device(boxes.device):
        keep_dev = torch.empty(n, dtype=torch.int64, device=boxes.device)
        k = wnms_sorted(boxes, data2merge_score, output, keep_dev, count, nms_thresh, merge_thresh, _SEMANTICS)
        keep[:k].copy_(keep_dev[:k])  # device -> host, synchronous
    return k
