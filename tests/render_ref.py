"""NumPy restatement of the debug panels as ``include/rv3d_render.h`` declares them: the scalar planes, min-max
normalisation and colour lookup, the bird's-eye view (point splat, footprint polylines with the declared integer raster rule), the
panel layout of ``draw_detections`` and the fp64 3-D IoU.  Slow and plain on purpose: one pixel, one box, one segment at a time where
that is how the rule reads.  ``tests/test_render_cpu.py`` checks it against the reference's own functions (``tests/golden/render/``);
the GPU tests compare the kernels to it, and ``profiles/tools/ab_render.py`` times it as the host route."""

from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

F = np.float32
RED, GREEN, BLUE = 1, 2, 4  # channel bits of rv_render_bev_boxes
IOU_GREEN = F(0.7)


# ----------------------------------------------------------------------------------------------------------------------
# A.1 scalar planes
# ----------------------------------------------------------------------------------------------------------------------
def plane_norm(cart) -> np.ndarray:
    x, y, z = (np.asarray(c, F) for c in cart)
    return np.sqrt((x * x + y * y) + z * z, dtype=F)


def plane_abs(x) -> np.ndarray:
    return np.abs(np.asarray(x, F))


def plane_likelihood64(logits) -> np.ndarray:
    """float64 of the same fp32 logits: what the device's fp32 plane is compared to."""
    m = np.asarray(logits, F).max(axis=0).astype(np.float64)
    return 1.0 / (1.0 + np.exp(-m))


def plane_likelihood(logits) -> np.ndarray:
    """fp32, NumPy's expf (the host route; the last bits are the library's)."""
    m = np.asarray(logits, F).max(axis=0)
    return (F(1.0) / (F(1.0) + np.exp(-m, dtype=F))).astype(F)


# ----------------------------------------------------------------------------------------------------------------------
# A.2 normalize_apply_colormap
# ----------------------------------------------------------------------------------------------------------------------
def colormap_index(plane) -> np.ndarray:
    p = np.asarray(plane, F)
    lo, hi = p.min(), p.max()
    den = F(F(hi - lo) + F(1e-6))
    v = ((p - lo) / den).astype(F) * F(255.0)
    return np.clip(np.nan_to_num(v, nan=0.0), 0, 255).astype(np.int64)


def normalize_apply_colormap(plane, lut, mask=None) -> np.ndarray:
    """(H,W) fp32, lut (3,256) u8, mask (H,W) or None -> (3,H,W) u8."""
    rgb = np.asarray(lut, np.uint8)[:, colormap_index(plane)]
    if mask is not None:
        rgb = rgb * (np.asarray(mask).reshape(rgb.shape[1:]) != 0).astype(np.uint8)
    return rgb


# ----------------------------------------------------------------------------------------------------------------------
# A.4 bird's-eye view: points
# ----------------------------------------------------------------------------------------------------------------------
def bev_side(max_side: float, meter_per_px: float) -> int:
    return int(math.ceil(max_side * 2 / meter_per_px))


def world_to_image(v, max_side: float, meter_per_px: float) -> Tuple[np.ndarray, np.ndarray]:
    """One coordinate: (kept, floor(size - u)) with u = (v + max_side) / meter_per_px, all fp32."""
    with np.errstate(invalid="ignore"):
        u = ((np.asarray(v, F) + F(max_side)) / F(meter_per_px)).astype(F)
        upper, size = F(max_side / meter_per_px * 2.0), F(max_side * 2.0 / meter_per_px)
        return (u > 0) & (u < upper), np.floor(size - u)


def bev_points(cart, max_side: float, meter_per_px: float) -> np.ndarray:
    """cart (3, ...) fp32 -> (3, side, side) u8."""
    side = bev_side(max_side, meter_per_px)
    x, y, z = (np.asarray(c, F).reshape(-1) for c in cart)
    kx, r = world_to_image(x, max_side, meter_per_px)
    ky, c = world_to_image(y, max_side, meter_per_px)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = (plane_norm((x, y, z)) > 0) & kx & ky & (r >= 0) & (r < side) & (c >= 0) & (c < side)
    bev = np.zeros((3, side, side), np.uint8)
    bev[:, r[keep].astype(np.int64), c[keep].astype(np.int64)] = 255
    return bev


# ----------------------------------------------------------------------------------------------------------------------
# A.5 bird's-eye view: boxes
# ----------------------------------------------------------------------------------------------------------------------
def footprint_pixels(box, max_side: float, meter_per_px: float) -> List[Tuple[int, int]]:
    """(row, col) of the kept corners 6, 2, 3, 7 (rear-right, front-right, front-left, rear-left), in that order."""
    b = np.asarray(box, F)
    hl, hw = F(0.5) * b[3], F(0.5) * b[4]
    s, c = F(math.sin(float(b[6]))), F(math.cos(float(b[6])))
    pts = []
    for ux, uy in ((-hl, -hw), (hl, -hw), (hl, hw), (-hl, hw)):
        x = b[0] + (F(ux * c) - F(uy * s))
        y = b[1] + (F(ux * s) + F(uy * c))
        (kx, r), (ky, cc) = world_to_image(x, max_side, meter_per_px), world_to_image(y, max_side, meter_per_px)
        if kx and ky:
            pts.append((int(r), int(cc)))
    return pts


def on_segment(p, a, b) -> bool:
    """The declared rule, literally: |(p - a) L2 - t d|^2 <= L2^2, t = clamp((p - a).d, 0, L2); |p - a|^2 <= 1 for L2 == 0."""
    d = (b[0] - a[0], b[1] - a[1])
    e = (p[0] - a[0], p[1] - a[1])
    L2 = d[0] * d[0] + d[1] * d[1]  # (Python integers: no overflow)
    if L2 == 0:
        return e[0] * e[0] + e[1] * e[1] <= 1
    t = min(max(e[0] * d[0] + e[1] * d[1], 0), L2)
    v = (e[0] * L2 - t * d[0], e[1] * L2 - t * d[1])
    return v[0] * v[0] + v[1] * v[1] <= L2 * L2


def segment_pixels(a, b, side: int) -> List[Tuple[int, int]]:
    """The pixels of the segment: the rule over the bounding box grown by one pixel and clipped to the view (``on_segment`` on every
    pixel of the box, evaluated for all of them at once in int64: side <= 1024 keeps L2^2 |p - a|^2 below 2^63)."""
    assert side <= 1024
    r0, r1 = max(min(a[0], b[0]) - 1, 0), min(max(a[0], b[0]) + 1, side - 1)
    c0, c1 = max(min(a[1], b[1]) - 1, 0), min(max(a[1], b[1]) + 1, side - 1)
    if r1 < r0 or c1 < c0:
        return []
    r, c = np.meshgrid(np.arange(r0, r1 + 1, dtype=np.int64), np.arange(c0, c1 + 1, dtype=np.int64), indexing="ij")
    d0, d1, e0, e1 = b[0] - a[0], b[1] - a[1], r - a[0], c - a[1]
    L2 = d0 * d0 + d1 * d1
    if L2 == 0:
        hit = e0 * e0 + e1 * e1 <= 1
    else:
        t = np.clip(e0 * d0 + e1 * d1, 0, L2)
        v0, v1 = e0 * L2 - t * d0, e1 * L2 - t * d1
        hit = v0 * v0 + v1 * v1 <= L2 * L2
    return [(int(x), int(y)) for x, y in zip(r[hit], c[hit])]


def box_value(score) -> int:
    return int(np.clip(np.rint(F(255.0) * F(score)), 0, 255))


def draw_boxes(bev, boxes, scores, channels, max_side: float, meter_per_px: float) -> np.ndarray:
    """Draws on a copy of ``bev`` (3, side, side) in row order; a later box overwrites an earlier one."""
    out = np.array(bev, np.uint8)
    side = out.shape[1]
    for k, box in enumerate(np.asarray(boxes, F).reshape(-1, 7)):
        pts = footprint_pixels(box, max_side, meter_per_px)
        value = box_value(1.0 if scores is None else scores[k])
        rgb = [value if (int(channels[k]) >> ch) & 1 else 0 for ch in range(3)]
        for a, b in zip(pts[:-1], pts[1:]):
            for r, c in segment_pixels(a, b, side):
                out[:, r, c] = rgb
    return out


def detection_channels(best_iou) -> np.ndarray:
    return np.where(np.asarray(best_iou, F) >= IOU_GREEN, GREEN, RED).astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# A.6 3-D IoU, float64 (z = the box centre)
# ----------------------------------------------------------------------------------------------------------------------
def boxes_iou3d64(a, b) -> np.ndarray:
    from waymo_eval_ref import iou_pair

    a, b = np.asarray(a, F).reshape(-1, 7), np.asarray(b, F).reshape(-1, 7)
    out = np.zeros((len(a), len(b)), np.float64)
    # pairs whose circumscribed circles are apart have no intersection: skip the clip
    reach = 0.5 * (np.hypot(a[:, 3], a[:, 4]).astype(np.float64)[:, None] + np.hypot(b[:, 3], b[:, 4]).astype(np.float64)[None])
    d2 = (a[:, None, 0].astype(np.float64) - b[None, :, 0]) ** 2 + (a[:, None, 1].astype(np.float64) - b[None, :, 1]) ** 2
    for i, j in zip(*np.nonzero(d2 <= reach * reach * 1.01 + 1e-3)):
        out[i, j] = iou_pair(a[i], b[j])[1]
    return out


# ----------------------------------------------------------------------------------------------------------------------
# draw_detections: layout and composition
# ----------------------------------------------------------------------------------------------------------------------
def panel_list(head: Dict, aux: Optional[Dict]) -> List[Tuple]:
    """The panels in order: (stride, kind, task, key, channel), kind in {"likelihood", "aux", "range"} (tensorboard.py:272-425)."""
    panels = []
    for stride, level in head.items():
        tasks = [t for t in level if isinstance(t, int)]
        if stride == 1:
            panels += [(stride, "likelihood", t, None, None) for t in tasks]
            if aux is not None:
                for t, entries in aux[stride].items():
                    if isinstance(t, int):
                        panels += [(stride, "aux", t, k, ch) for k, v in entries.items() for ch in range(v.shape[1])]
        panels.append((stride, "range", None, None, None))
        panels += [(stride, "likelihood", t, None, None) for t in tasks]
    return panels


def compose(sizes_kinds: Sequence[Tuple[str, int, int]], side: int):
    """``sizes_kinds``: (kind, H, W) per panel in order.  Returns (H_total, W_total, origins, bev_origin): every panel's and the BEV's
    (row0, col0) in the stacked image.  Follows tensorboard.py: SW starts as the BEV's side; a panel with W < SW is padded to SW with
    left = (SW - W) // 2; at a level's range panel with W >= SW the BEV is padded to W with left = (W - SW) // 2 (its content moves
    right by that much) and SW becomes W.  All rows then have the width W_total, as torch.cat requires."""
    sw, bev_col, origins, widths, row = side, 0, [], [], 0
    for kind, h, w in sizes_kinds:
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
    if any(wd != sw for wd in widths):
        raise ValueError(f"the panels do not stack: widths {sorted(set(widths))} against the bird's-eye view's {sw}")
    return row + side, sw, origins, (row, bev_col)


def stack(panels_rgb: Sequence[np.ndarray], kinds: Sequence[str], bev: np.ndarray) -> np.ndarray:
    """The stacked (3, H_total, W_total) image of the coloured panels and the BEV."""
    side = bev.shape[1]
    H, W, origins, (br, bc) = compose([(k, p.shape[1], p.shape[2]) for k, p in zip(kinds, panels_rgb)], side)
    img = np.zeros((3, H, W), np.uint8)
    for p, (r, c) in zip(panels_rgb, origins):
        img[:, r:r + p.shape[1], c:c + p.shape[2]] = p
    img[:, br:br + side, bc:bc + side] = bev
    return img
