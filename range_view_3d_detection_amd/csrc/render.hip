// render.hip -- the training loop's debug panels (rendering/tensorboard.py of the reference: to_logger / draw_detections) and mmcv's
// IoU ops (compat/mmcv_ops.py), on tensors that already sit in HBM.  Declared semantics: include/rv3d_render.h.
//
//   rv_render_plane       plane_kernel: (C,H,W) fp32 -> (H,W) fp32 by norm / likelihood / abs / identity, and the plane's minimum and maximum
//                         (order-preserving integer keys, one atomicMax pair per wave: the result does not depend on the order)
//   rv_render_colormap    colormap_kernel: plane -> min-max normalised index -> LUT * mask, into a block of the planar uint8 image
//   rv_render_bev_points  bev_points_kernel: the point splat (every store writes 255: no order to decide)
//   rv_render_bev_boxes   bev_raster_kernel (one workgroup per box, threads over the bounding box of each footprint segment,
//                         atomicMax of the draw index on a side x side u32 image: the z-buffer idiom of project.hip and dbsample.hip)
//                         + bev_resolve_kernel (one thread per pixel: the colour of the last box drawn there)
//   rv_boxes_iou3d        boxes_iou3d_kernel: one thread per pair, waymo_iou_pair of nms_geom.h
//   rv_rotated_iou_pairs  rotated_iou_pairs_kernel: one thread per ALIGNED pair, rotated_iou of nms_geom.h
//
// Plain HIP C++, every loop bounded by an image or a row count, no workgroup waits for another.  Built without fused multiply-add
// contraction (csrc/Makefile, EXACT): every step of the declared arithmetic is one fp32 IEEE operation.
#include "common.h"

#include <math.h>

#include "../../include/rv3d_render.h"
#include "colormaps.h"
#include "nms_geom.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_SIDE_PX = 4096;  // BEV side: the integer raster test stays far inside int64 (see on_segment)

const uint8_t h_cmaps[3][768] = {RV_CMAP_GREYS_INIT, RV_CMAP_TURBO_R_INIT, RV_CMAP_VIRIDIS_INIT};

// order-preserving map fp32 -> u32 (and back): a < b <=> key(a) < key(b) for non-NaN values, -0 < +0
__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// minmax[0] = max of ~key (the minimum), minmax[1] = max of key (the maximum); both start at 0
__global__ __launch_bounds__(THREADS) void plane_kernel(const float* src, int64_t channel_stride, int C, int64_t n, int op, float* plane,
                                                        uint32_t* minmax) {
    uint32_t lo = 0, hi = 0;
    for (int64_t i = blockIdx.x * (int64_t)THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        float v;
        if (op == RV_PLANE_NORM) {
            const float x = src[i], y = src[channel_stride + i], z = src[2 * channel_stride + i];
            v = sqrtf((x * x + y * y) + z * z);
        } else if (op == RV_PLANE_LIKELIHOOD) {
            float m = src[i];
            for (int c = 1; c < C; ++c) m = fmaxf(m, src[c * channel_stride + i]);
            v = 1.0f / (1.0f + expf(-m));
        } else if (op == RV_PLANE_ABS) {
            v = fabsf(src[i]);
        } else {
            v = src[i];
        }
        plane[i] = v;
        const uint32_t k = key_of(v);
        lo = ~k > lo ? ~k : lo;
        hi = k > hi ? k : hi;
    }
    lo = wave_max_u32(lo), hi = wave_max_u32(hi);
    if ((threadIdx.x & 63) == 0) {
        if (lo) atomicMax(minmax, lo);
        if (hi) atomicMax(minmax + 1, hi);
    }
}

__global__ __launch_bounds__(THREADS) void colormap_kernel(const float* plane, const uint8_t* mask, int H, int W, const uint32_t* minmax,
                                                           const uint8_t* lut, uint8_t* image, int64_t image_plane, int W_total, int row0,
                                                           int col0) {
    const float lo = float_of(~minmax[0]), hi = float_of(minmax[1]);
    const float den = (hi - lo) + 1e-6f;
    const int64_t n = (int64_t)H * W;
    for (int64_t i = blockIdx.x * (int64_t)THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const float v = ((plane[i] - lo) / den) * 255.0f;
        const int idx = v >= 0.0f ? (v < 255.0f ? (int)v : 255) : 0;  // (a NaN takes index 0)
        const uint8_t keep = mask ? (mask[i] != 0) : 1;
        const int r = (int)(i / W), c = (int)(i - (int64_t)r * W);
        const int64_t at = (int64_t)(row0 + r) * W_total + (col0 + c);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) image[ch * image_plane + at] = (uint8_t)(lut[ch * 256 + idx] * keep);
    }
}

// world_to_image of one coordinate: u = (v + max_side) / meter_per_px, kept iff 0 < u < upper, pixel = floor(size - u)
struct BevMap {
    float max_side, meter_per_px, upper, size;
};
__device__ __forceinline__ bool bev_map(const BevMap& m, float v, float& px) {
    const float u = (v + m.max_side) / m.meter_per_px;
    px = floorf(m.size - u);
    return u > 0.0f && u < m.upper;
}

__global__ __launch_bounds__(THREADS) void bev_points_kernel(const float* cart, int64_t channel_stride, int64_t n, BevMap m, int side,
                                                             uint8_t* image, int64_t image_plane, int W_total, int row0, int col0) {
    for (int64_t i = blockIdx.x * (int64_t)THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const float x = cart[i], y = cart[channel_stride + i], z = cart[2 * channel_stride + i];
        if (!(sqrtf((x * x + y * y) + z * z) > 0.0f)) continue;
        float fr, fc;
        const bool kx = bev_map(m, x, fr), ky = bev_map(m, y, fc);
        if (!(kx && ky)) continue;
        if (!(fr >= 0.0f && fr < (float)side && fc >= 0.0f && fc < (float)side)) continue;  // (`side` itself: the reference would raise)
        const int64_t at = (int64_t)(row0 + (int)fr) * W_total + (col0 + (int)fc);
        image[at] = 255, image[image_plane + at] = 255, image[2 * image_plane + at] = 255;
    }
}

// The declared raster rule: pixel p belongs to the segment a -> b iff |(p - a) L2 - t d|^2 <= L2^2 with d = b - a, L2 = d.d,
// t = clamp((p - a).d, 0, L2); |p - a|^2 <= 1 for L2 == 0.  Evaluated in its three exact integer cases, which cannot overflow:
// t = 0: |p - a|^2 L2^2 <= L2^2;  t = L2: |p - b|^2 L2^2 <= L2^2;  else |(p - a) L2 - t d|^2 = L2 ((p - a) x d)^2 <= L2^2.
__device__ __forceinline__ bool on_segment(int64_t pr, int64_t pc, int64_t ar, int64_t ac, int64_t br, int64_t bc) {
    const int64_t dr = br - ar, dc = bc - ac, er = pr - ar, ec = pc - ac;
    const int64_t L2 = dr * dr + dc * dc, s = er * dr + ec * dc;
    if (L2 == 0 || s <= 0) return er * er + ec * ec <= 1;
    if (s >= L2) return (pr - br) * (pr - br) + (pc - bc) * (pc - bc) <= 1;
    const int64_t cr = er * dc - ec * dr;
    return cr * cr <= L2;
}

__global__ __launch_bounds__(THREADS) void bev_raster_kernel(const float* boxes, int64_t n, BevMap m, int side, uint32_t* zbuf) {
    __shared__ int pts[4][2];
    __shared__ int n_pts;
    const int64_t k = blockIdx.x;
    if (k >= n) return;
    if (threadIdx.x == 0) {
        const float* b = boxes + k * 7;
        const float hl = 0.5f * b[3], hw = 0.5f * b[4];
        float s, c;
        yaw_sincos(b[6], s, c);
        // corners 6, 2, 3, 7 of cuboids_to_vertices: rear-right, front-right, front-left, rear-left
        const float ux[4] = {-hl, hl, hl, -hl}, uy[4] = {-hw, -hw, hw, hw};
        int cnt = 0;
        for (int v = 0; v < 4; ++v) {
            const float x = b[0] + (ux[v] * c - uy[v] * s), y = b[1] + (ux[v] * s + uy[v] * c);
            float fr, fc;
            const bool kx = bev_map(m, x, fr), ky = bev_map(m, y, fc);
            if (kx && ky) pts[cnt][0] = (int)fr, pts[cnt][1] = (int)fc, ++cnt;  // (kept: |fr|, |fc| <= size + 1, the cast is exact)
        }
        n_pts = cnt;
    }
    __syncthreads();
    const uint32_t draw = (uint32_t)(k + 1);
    for (int e = 0; e + 1 < n_pts; ++e) {
        const int ar = pts[e][0], ac = pts[e][1], br = pts[e + 1][0], bc = pts[e + 1][1];
        int r0 = (ar < br ? ar : br) - 1, r1 = (ar > br ? ar : br) + 1, c0 = (ac < bc ? ac : bc) - 1, c1 = (ac > bc ? ac : bc) + 1;
        r0 = r0 < 0 ? 0 : r0, c0 = c0 < 0 ? 0 : c0, r1 = r1 > side - 1 ? side - 1 : r1, c1 = c1 > side - 1 ? side - 1 : c1;
        if (r1 < r0 || c1 < c0) continue;
        const int w = c1 - c0 + 1, cells = (r1 - r0 + 1) * w;  // <= side * side
        for (int q = threadIdx.x; q < cells; q += THREADS) {
            const int pr = r0 + q / w, pc = c0 + q % w;
            if (on_segment(pr, pc, ar, ac, br, bc)) atomicMax(zbuf + (int64_t)pr * side + pc, draw);
        }
    }
}

__global__ __launch_bounds__(THREADS) void bev_resolve_kernel(const uint32_t* zbuf, const float* scores, const uint8_t* channels, int64_t n,
                                                              int side, uint8_t* image, int64_t image_plane, int W_total, int row0,
                                                              int col0) {
    const int64_t cells = (int64_t)side * side;
    for (int64_t i = blockIdx.x * (int64_t)THREADS + threadIdx.x; i < cells; i += (int64_t)gridDim.x * THREADS) {
        const uint32_t draw = zbuf[i];
        if (draw == 0 || (int64_t)draw > n) continue;
        const float f = rintf(255.0f * (scores ? scores[draw - 1] : 1.0f));
        const uint8_t value = f >= 0.0f ? (f < 255.0f ? (uint8_t)f : 255) : 0;  // (saturating, a NaN draws 0)
        const uint8_t chan = channels[draw - 1];
        const int r = (int)(i / side), c = (int)(i - (int64_t)r * side);
        const int64_t at = (int64_t)(row0 + r) * W_total + (col0 + c);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) image[ch * image_plane + at] = ((chan >> ch) & 1) ? value : 0;
    }
}

__global__ __launch_bounds__(THREADS) void boxes_iou3d_kernel(const float* a, int64_t n, const float* b, int64_t m, float* out) {
    const int64_t total = n * m;
    for (int64_t k = blockIdx.x * (int64_t)THREADS + threadIdx.x; k < total; k += (int64_t)gridDim.x * THREADS) {
        const int64_t i = k / m, j = k - i * m;
        out[k] = waymo_iou_pair(a + i * 7, b + j * 7).y;
    }
}

__global__ __launch_bounds__(THREADS) void rotated_iou_pairs_kernel(const float* a, const float* b, int64_t n, float* out) {
    for (int64_t k = blockIdx.x * (int64_t)THREADS + threadIdx.x; k < n; k += (int64_t)gridDim.x * THREADS) {
        float sa, ca, sb, cb;
        yaw_sincos(a[k * 5 + 4], sa, ca);
        yaw_sincos(b[k * 5 + 4], sb, cb);
        out[k] = rotated_iou(a + k * 5, sa, ca, b + k * 5, sb, cb);
    }
}

inline unsigned grid_of(int64_t n) {
    const int64_t blocks = (n + THREADS - 1) / THREADS;
    return (unsigned)(blocks < 4096 ? (blocks < 1 ? 1 : blocks) : 4096);
}

// the block [row0, row0 + h) x [col0, col0 + w) lies inside the (3, H_total, W_total) image
inline bool block_fits(int64_t h, int64_t w, int64_t H_total, int64_t W_total, int64_t row0, int64_t col0) {
    return H_total > 0 && W_total > 0 && H_total * W_total <= 0x7fffffff && row0 >= 0 && col0 >= 0 && row0 + h <= H_total && col0 + w <= W_total;
}

inline int bev_setup(const char* who, double max_side, double meter_per_px, int32_t side, BevMap* m) {
    RV_REQUIRE(max_side > 0.0 && meter_per_px > 0.0 && side >= 1 && side <= MAX_SIDE_PX, "%s: max_side %g, meter_per_px %g, side %d (1 .. %d)", who,
               max_side, meter_per_px, (int)side, MAX_SIDE_PX);
    // the reference's Python (fp64) expressions, rounded to fp32 where they meet the fp32 tensor
    m->max_side = (float)max_side, m->meter_per_px = (float)meter_per_px;
    m->upper = (float)(max_side / meter_per_px * 2.0), m->size = (float)(max_side * 2.0 / meter_per_px);
    return 0;
}

}  // namespace

extern "C" int rv_render_colormap_table(int32_t table, uint8_t* host_out) {
    RV_REQUIRE(table >= 0 && table < 3 && host_out, "rv_render_colormap_table: table %d (0 .. 2) or a null buffer", (int)table);
    memcpy(host_out, h_cmaps[table], 768);
    return 0;
}

extern "C" int rv_render_plane(const float* src, int64_t channel_stride, int32_t C, int32_t H, int32_t W, int32_t op, float* plane,
                               void* minmax, rvStream stream) {
    RV_REQUIRE(src && plane && minmax, "rv_render_plane: null argument");
    RV_REQUIRE(H > 0 && W > 0 && C >= 1 && channel_stride >= (int64_t)H * W, "rv_render_plane: C %d, H %d, W %d, channel stride %lld", (int)C,
               (int)H, (int)W, (long long)channel_stride);
    RV_REQUIRE(op >= RV_PLANE_NORM && op <= RV_PLANE_IDENTITY, "rv_render_plane: unknown op %d", (int)op);
    RV_REQUIRE(op != RV_PLANE_NORM || C == 3, "rv_render_plane: norm takes 3 channels, got %d", (int)C);
    RV_REQUIRE((op != RV_PLANE_ABS && op != RV_PLANE_IDENTITY) || C == 1, "rv_render_plane: abs / identity take 1 channel, got %d", (int)C);
    RV_REQUIRE((uintptr_t)minmax % 4 == 0, "rv_render_plane: minmax must be 4-byte aligned");
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(plane_kernel, dim3(grid_of(n)), dim3(THREADS), 0, (hipStream_t)stream, src, channel_stride, (int)C, n, (int)op, plane,
                       (uint32_t*)minmax);
    RV_CHECK_LAUNCH("plane_kernel");
    return 0;
}

extern "C" int rv_render_colormap(const float* plane, const uint8_t* mask, int32_t H, int32_t W, const void* minmax, const uint8_t* lut,
                                  uint8_t* image, int32_t H_total, int32_t W_total, int32_t row0, int32_t col0, rvStream stream) {
    RV_REQUIRE(plane && minmax && lut && image, "rv_render_colormap: null argument");
    RV_REQUIRE(H > 0 && W > 0 && block_fits(H, W, H_total, W_total, row0, col0),
               "rv_render_colormap: block %d x %d at (%d, %d) does not fit the image %d x %d", (int)H, (int)W, (int)row0, (int)col0, (int)H_total,
               (int)W_total);
    hipLaunchKernelGGL(colormap_kernel, dim3(grid_of((int64_t)H * W)), dim3(THREADS), 0, (hipStream_t)stream, plane, mask, (int)H, (int)W,
                       (const uint32_t*)minmax, lut, image, (int64_t)H_total * W_total, (int)W_total, (int)row0, (int)col0);
    RV_CHECK_LAUNCH("colormap_kernel");
    return 0;
}

extern "C" int rv_render_bev_points(const float* cart, int64_t channel_stride, int64_t n, double max_side, double meter_per_px, int32_t side,
                                    uint8_t* image, int32_t H_total, int32_t W_total, int32_t row0, int32_t col0, rvStream stream) {
    BevMap m;
    if (bev_setup("rv_render_bev_points", max_side, meter_per_px, side, &m)) return 1;
    RV_REQUIRE(n >= 0 && channel_stride >= n, "rv_render_bev_points: n %lld, channel stride %lld", (long long)n, (long long)channel_stride);
    RV_REQUIRE(image && block_fits(side, side, H_total, W_total, row0, col0),
               "rv_render_bev_points: null image, or the %d x %d view at (%d, %d) does not fit the image %d x %d", (int)side, (int)side, (int)row0,
               (int)col0, (int)H_total, (int)W_total);
    if (n == 0) return 0;
    RV_REQUIRE(cart, "rv_render_bev_points: null points");
    hipLaunchKernelGGL(bev_points_kernel, dim3(grid_of(n)), dim3(THREADS), 0, (hipStream_t)stream, cart, channel_stride, n, m, (int)side, image,
                       (int64_t)H_total * W_total, (int)W_total, (int)row0, (int)col0);
    RV_CHECK_LAUNCH("bev_points_kernel");
    return 0;
}

extern "C" int rv_render_bev_boxes(const float* boxes, const float* scores, const uint8_t* channels, int64_t n, double max_side,
                                   double meter_per_px, int32_t side, void* zbuf, uint8_t* image, int32_t H_total, int32_t W_total,
                                   int32_t row0, int32_t col0, rvStream stream) {
    BevMap m;
    if (bev_setup("rv_render_bev_boxes", max_side, meter_per_px, side, &m)) return 1;
    RV_REQUIRE(n >= 0 && n <= 0x7ffffff, "rv_render_bev_boxes: %lld boxes", (long long)n);
    RV_REQUIRE(image && block_fits(side, side, H_total, W_total, row0, col0),
               "rv_render_bev_boxes: null image, or the %d x %d view at (%d, %d) does not fit the image %d x %d", (int)side, (int)side, (int)row0,
               (int)col0, (int)H_total, (int)W_total);
    if (n == 0) return 0;
    RV_REQUIRE(boxes && channels && zbuf && (uintptr_t)zbuf % 4 == 0, "rv_render_bev_boxes: null boxes, channels or z-buffer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t cells = (int64_t)side * side;
    hipError_t e = hipMemsetAsync(zbuf, 0, (size_t)cells * 4, st);
    if (e != hipSuccess) RV_FAIL("rv_render_bev_boxes: clearing the z-buffer: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(bev_raster_kernel, dim3((unsigned)n), dim3(THREADS), 0, st, boxes, n, m, (int)side, (uint32_t*)zbuf);
    hipLaunchKernelGGL(bev_resolve_kernel, dim3(grid_of(cells)), dim3(THREADS), 0, st, (const uint32_t*)zbuf, scores, channels, n, (int)side,
                       image, (int64_t)H_total * W_total, (int)W_total, (int)row0, (int)col0);
    RV_CHECK_LAUNCH("bev box kernels");
    return 0;
}

extern "C" int rv_boxes_iou3d(const float* a, int64_t n, const float* b, int64_t m, float* out, rvStream stream) {
    RV_REQUIRE(n >= 0 && m >= 0 && n <= 0x7fffffff && m <= 0x7fffffff, "rv_boxes_iou3d: n = %lld, m = %lld", (long long)n, (long long)m);
    if (n * m == 0) return 0;
    RV_REQUIRE(a && b && out, "rv_boxes_iou3d: null argument");
    hipLaunchKernelGGL(boxes_iou3d_kernel, dim3(grid_of(n * m)), dim3(THREADS), 0, (hipStream_t)stream, a, n, b, m, out);
    RV_CHECK_LAUNCH("boxes_iou3d_kernel");
    return 0;
}

extern "C" int rv_rotated_iou_pairs(const float* a, const float* b, int64_t n, float* out, rvStream stream) {
    RV_REQUIRE(n >= 0, "rv_rotated_iou_pairs: n = %lld", (long long)n);
    if (n == 0) return 0;
    RV_REQUIRE(a && b && out, "rv_rotated_iou_pairs: null argument");
    hipLaunchKernelGGL(rotated_iou_pairs_kernel, dim3(grid_of(n)), dim3(THREADS), 0, (hipStream_t)stream, a, b, n, out);
    RV_CHECK_LAUNCH("rotated_iou_pairs_kernel");
    return 0;
}
