"""``nms_mode: HARD`` restated in numpy over ``oracle.nms.pairwise_iou`` (helper of the hard-NMS tests, not a test module).

Declared semantics (``include/rv3d.h``): walk the boxes of a class in descending score order, equal scores in ascending input
index; a box not yet suppressed is kept; a kept box suppresses every later box whose rotated BEV IoU with it is strictly
greater than the threshold; a suppressed box suppresses nothing.  Wrapper logic as the reference's ``hard_multiclass_nms`` /
``batched_multiclass_nms`` (``math/ops/nms.py:10-61, 181-266``): ``score >= min_confidence`` per sweep, classes ascending,
the ``num_pre_nms`` best of the class, NMS, the first ``num_post_nms`` kept rows.  Everything is returned as INDICES into the
input, so that a caller can require output rows to be input rows bit for bit.  The CPU IoU equals the device's bit for bit
(same unfused fp32 arithmetic), so comparisons against the device are exact.
"""

from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from oracle import nms as onms


def rect_of(cuboids: np.ndarray) -> np.ndarray:
    """(n,7) [x,y,z,l,w,h,yaw] -> (n,5) [x - l/2, y - w/2, x + l/2, y + w/2, yaw], fp32 (the weighted path's rectangle)."""
    c = np.asarray(cuboids, dtype=np.float32)
    hl, hw = c[:, 3] / np.float32(2), c[:, 4] / np.float32(2)
    return np.stack([c[:, 0] - hl, c[:, 1] - hw, c[:, 0] + hl, c[:, 1] + hw, c[:, 6]], axis=1).astype(np.float32)


def score_order(scores: np.ndarray) -> np.ndarray:
    """Descending score, ascending index on ties."""
    return np.argsort(-np.asarray(scores, dtype=np.float32), kind="stable")


def nms_sorted(rect: np.ndarray, iou_threshold: float) -> np.ndarray:
    """Score-sorted rectangles -> sorted positions of the kept boxes, ascending.  One IoU row per KEPT box, over the boxes still
    alive behind it."""
    n = rect.shape[0]
    alive = np.ones(n, dtype=bool)
    thr = np.float32(iou_threshold)
    keep: List[int] = []
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        later = i + 1 + np.flatnonzero(alive[i + 1:])
        if later.size:
            iou = onms.pairwise_iou(rect[i:i + 1], rect[later])[0]
            alive[later[iou > thr]] = False
    return np.asarray(keep, dtype=np.int64)


def nms_rotated(boxes: np.ndarray, scores: np.ndarray, iou_threshold: float) -> np.ndarray:
    """detectron2's signature: unsorted (n,5) ``(cx, cy, w, h, degrees)`` and (n,) scores -> kept indices, descending score.  The angle
    runs counter-clockwise in image coordinates (y down): the rectangle's ``ry`` is ``-angle`` in radians."""
    b = np.asarray(boxes, dtype=np.float32)
    order = score_order(scores)
    b = b[order]
    half = b[:, 2:4] / np.float32(2)
    ry = (torch.from_numpy(b[:, 4:5].copy()) * (-np.pi / 180.0)).numpy()  # fp32 tensor times a Python scalar, as the shim computes it
    rect = np.concatenate([b[:, :2] - half, b[:, :2] + half, ry], axis=1).astype(np.float32)
    return order[nms_sorted(rect, iou_threshold)]


def hard_multiclass(cuboids: np.ndarray, scores: np.ndarray, cats: np.ndarray, iou_threshold: float, num_pre_nms: int,
                    num_post_nms: int) -> Tuple[np.ndarray, np.ndarray]:
    """One sweep (already filtered by confidence): indices of the output rows in output order, and their classes."""
    rows, classes = [], []
    for j in np.unique(cats):
        idx = np.flatnonzero(cats == j)
        idx = idx[score_order(scores[idx])][:num_pre_nms]
        keep = nms_sorted(rect_of(cuboids[idx]), iou_threshold)[:num_post_nms]
        rows.append(idx[keep])
        classes.append(np.full(keep.size, j, dtype=np.int64))
    if not rows:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(rows), np.concatenate(classes)


def batched(cuboids, scores, cats, num_pre_nms: int, num_post_nms: int, iou_threshold: float, min_confidence: float):
    """(B,K,7), (B,K), (B,K) tensors or arrays -> (sweep index, candidate index, class) of every output row, in output order."""
    cub, sc, ct = (np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in (cuboids, scores, cats))
    bi, ki, ci = [], [], []
    for b in range(sc.shape[0]):
        m = np.flatnonzero(sc[b] >= np.float32(min_confidence))
        if m.size == 0:
            continue
        rows, classes = hard_multiclass(cub[b, m], sc[b, m], ct[b, m], iou_threshold, num_pre_nms, num_post_nms)
        bi.append(np.full(rows.size, b, dtype=np.int64))
        ki.append(m[rows])
        ci.append(classes)
    if not bi:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    return np.concatenate(bi), np.concatenate(ki), np.concatenate(ci)


def batched_rows(cuboids: torch.Tensor, scores: torch.Tensor, cats: torch.Tensor, *cfg):
    """The four tensors ``batched_multiclass_nms(nms_mode="HARD")`` returns: input rows, input scores, float classes and batch index."""
    bi, ki, ci = batched(cuboids, scores, cats, *cfg)
    cub, sc = cuboids.cpu(), scores.cpu()
    if bi.size == 0:
        return cub.new_empty((0, cub.shape[-1])), sc.new_empty((0, 1)), cats.cpu().new_empty((0, 1)), cats.cpu().new_empty((0, 1))
    bi, ki = torch.from_numpy(bi), torch.from_numpy(ki)
    return cub[bi, ki], sc[bi, ki], torch.from_numpy(ci).to(sc.dtype), bi.to(sc.dtype)


def canonical(p, s, c, b):
    """Rows with exactly equal (sweep, class, score) leave ``topk`` in an order torch does not define; the device breaks such ties by
    candidate index.  Inside a tie group the rows are compared as a set: ordered by box centre here (as tests/test_gpu_nms_wrapper.py does)."""
    p, s, c, b = (t.detach().cpu() for t in (p, s, c, b))
    if s.dim() != 1 or s.numel() == 0:
        return p, s, c, b
    same = (s[1:] == s[:-1]) & (c[1:] == c[:-1]) & (b[1:] == b[:-1])
    group = torch.cat([torch.zeros(1, dtype=torch.long), (~same).long().cumsum(0)])
    order = torch.from_numpy(np.lexsort((p[:, 1].numpy(), p[:, 0].numpy(), group.numpy())))
    return p[order], s, c, b


def same_rows_exact(got, want, what):
    """Row order, classes, batch index, dtypes and shapes exact; boxes and scores bit for bit (ties canonicalised)."""
    p, s, c, b = canonical(*got)
    rp, rs, rc, rb = canonical(*want)
    assert p.shape == rp.shape and s.shape == rs.shape, (what, tuple(p.shape), tuple(rp.shape))
    assert c.dtype == rc.dtype and b.dtype == rb.dtype and p.dtype == rp.dtype and s.dtype == rs.dtype, what
    assert torch.equal(c, rc), f"{what}: categories / row order differ"
    assert torch.equal(b, rb), f"{what}: batch index differs"
    assert torch.equal(s, rs), f"{what}: scores differ"
    assert torch.equal(p, rp), f"{what}: boxes are not the selected input rows"
