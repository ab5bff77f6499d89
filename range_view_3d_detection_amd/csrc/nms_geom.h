// Rotated-BEV-IoU of two boxes [x1, y1, x2, y2, ry], the rectangle of a box and the sin / cos the IoU takes.  Users: nms_core.h (the
// pair masks of nms.hip and nms2.hip), nms.hip (sin / cos pass, rv_rotated_iou), nms2.hip (gather), softassign.hip (BEV affinity),
// evaluate_waymo.hip and render.hip (BEV / 3-D IoU); all include it where fused multiply-add contraction is off, so that the result matches
// oracle/c/oracle.c bit for bit.
#pragma once
#include "common.h"

namespace {

struct Pt {
    float x, y;
};

// [x1, y1, x2, y2, ry] of the BEV footprint of a box at (x, y), length l along +yaw, width w
__device__ __forceinline__ void rect_of_box(float x, float y, float l, float w, float yaw, float* r) {
    const float hl = 0.5f * l, hw = 0.5f * w;
    r[0] = x - hl, r[1] = y - hw, r[2] = x + hl, r[3] = y + hw, r[4] = yaw;
}

// the sin / cos of the IoU arithmetic: fp32 roundings of the fp64 values
__device__ __forceinline__ void yaw_sincos(float yaw, float& s, float& c) {
    s = (float)sin((double)yaw);
    c = (float)cos((double)yaw);
}

__device__ __forceinline__ float cross2(Pt a, Pt b, Pt p) { return (b.x - a.x) * (p.y - a.y) - (b.y - a.y) * (p.x - a.x); }

__device__ void corners(const float* b, float s, float c, Pt* out) {
    const float cx = (b[0] + b[2]) * 0.5f, cy = (b[1] + b[3]) * 0.5f;
    const float hx = (b[2] - b[0]) * 0.5f, hy = (b[3] - b[1]) * 0.5f;
    const float dx[4] = {hx, -hx, -hx, hx};
    const float dy[4] = {hy, hy, -hy, -hy};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        out[k].x = cx + (dx[k] * c - dy[k] * s);
        out[k].y = cy + (dx[k] * s + dy[k] * c);
    }
}

// rectangle A clipped by the four half-planes of rectangle B (Sutherland-Hodgman), shoelace area: the area of the intersection, 0
// when fewer than three vertices are left
__device__ __forceinline__ float rotated_intersection(const float* a, float sa, float ca, const float* b, float sb, float cb) {
    Pt pa[4], pb[4], poly[16], tmp[16];
    corners(a, sa, ca, pa);
    corners(b, sb, cb, pb);
    int n = 4;
    for (int k = 0; k < 4; ++k) poly[k] = pa[k];
    for (int e = 0; e < 4 && n > 0; ++e) {
        const Pt e0 = pb[e], e1 = pb[(e + 1) & 3];
        int m = 0;
        for (int k = 0; k < n; ++k) {
            const Pt p = poly[k], q = poly[(k + 1 == n) ? 0 : k + 1];
            const float dp = cross2(e0, e1, p), dq = cross2(e0, e1, q);
            const bool in_p = dp >= 0.0f, in_q = dq >= 0.0f;
            if (in_p) tmp[m++] = p;
            if (in_p != in_q) {
                const float t = dp / (dp - dq);
                Pt r;
                r.x = p.x + t * (q.x - p.x);
                r.y = p.y + t * (q.y - p.y);
                tmp[m++] = r;
            }
        }
        n = m;
        for (int k = 0; k < n; ++k) poly[k] = tmp[k];
    }
    if (n < 3) return 0.0f;
    float twice = 0.0f;
    for (int k = 0; k < n; ++k) {
        const Pt p = poly[k], q = poly[(k + 1 == n) ? 0 : k + 1];
        twice += (p.x - poly[0].x) * (q.y - poly[0].y) - (p.y - poly[0].y) * (q.x - poly[0].x);
    }
    return 0.5f * fabsf(twice);
}

// IoU of the two rectangles and, through `inter`, the intersection area it was formed from (0 where the IoU is 0 by one of the early
// exits; an empty intersection leaves early: 0 / uni would be the same +0)
__device__ __forceinline__ float rotated_iou_inter(const float* a, float sa, float ca, const float* b, float sb, float cb, float& inter) {
    inter = 0.0f;
    const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
    const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
    if (!(area_a > 0.0f) || !(area_b > 0.0f)) return 0.0f;
    inter = rotated_intersection(a, sa, ca, b, sb, cb);
    if (inter == 0.0f) return 0.0f;
    const float uni = area_a + area_b - inter;
    if (!(uni > 0.0f)) return 0.0f;
    return inter / uni;
}

__device__ float rotated_iou(const float* a, float sa, float ca, const float* b, float sb, float cb) {
    float inter;
    return rotated_iou_inter(a, sa, ca, b, sb, cb, inter);
}

// (BEV, 3-D) IoU of two boxes [x, y, z, l, w, h, yaw], z the CENTRE (include/rv3d.h, "IoU of a pair"): ONE function for
// waymo_iou_kernel (evaluate_waymo.hip) and boxes_iou3d_kernel (render.hip), so that the two agree bit for bit
__device__ float2 waymo_iou_pair(const float* a, const float* b) {
    float2 out = make_float2(0.0f, 0.0f);
    // circumscribed circles of the footprints apart (with a margin far above the rounding of the clip): the intersection is empty
    const float dx = a[0] - b[0], dy = a[1] - b[1];
    const float reach = 0.5f * (sqrtf(a[3] * a[3] + a[4] * a[4]) + sqrtf(b[3] * b[3] + b[4] * b[4]));
    if (dx * dx + dy * dy > reach * reach * 1.001f + 1e-6f) return out;
    float ra[5], rb[5], sa, ca, sb, cb, area;  // boxes are [x, y, z, l, w, h, yaw]; the rectangles rv_rotated_iou takes
    rect_of_box(a[0], a[1], a[3], a[4], a[6], ra), rect_of_box(b[0], b[1], b[3], b[4], b[6], rb);
    yaw_sincos(a[6], sa, ca), yaw_sincos(b[6], sb, cb);
    out.x = rotated_iou_inter(ra, sa, ca, rb, sb, cb, area);
    const float hha = 0.5f * a[5], hhb = 0.5f * b[5];
    const float top_a = a[2] + hha, top_b = b[2] + hhb, bot_a = a[2] - hha, bot_b = b[2] - hhb;
    const float top = top_a < top_b ? top_a : top_b, bot = bot_a > bot_b ? bot_a : bot_b;
    const float dz = top - bot > 0.0f ? top - bot : 0.0f;
    const float vol_a = (a[3] * a[4]) * a[5], vol_b = (b[3] * b[4]) * b[5];
    if (!(vol_a > 0.0f) || !(vol_b > 0.0f)) return out;
    const float inter = area * dz;
    const float uni = vol_a + vol_b - inter;
    if (uni > 0.0f) out.y = inter / uni;
    return out;
}

}  // namespace
