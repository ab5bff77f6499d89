// roi.hip -- AV2 region-of-interest (ROI) lookups and the ROI raster builder, on the device.
//
// The reference's AV2 converter flags every lidar return with av2's CPU map API (converters/av2/export.py:91-97:
// city_SE3_ego.transform_from, then get_raster_layer_points_boolean(ROI)), and its AV2 evaluation keeps only the boxes inside the ROI
// (datasets/__init__.py:29 eval_only_roi_instances, handed to av2's evaluate).  av2 is not part of the reference tree, so the semantics
// are DECLARED (include/rv3d.h) -- parity unpinned, as for rv_eval_match.  Entry points:
//
//   rv_roi_points     roi_points_kernel: one thread per point, grid-stride; the point's sweep by binary search in the CSR offsets.
//   rv_roi_boxes      roi_boxes_kernel: one thread per box, its 8 vertices through the same lookup; any vertex inside = inside.
//   rv_roi_rasterize  roi_bbox_kernel (one workgroup per polygon: bounding box in raster coordinates), roi_fill_kernel (one thread per
//                     pixel, a 64 x 4 tile per workgroup, polygons whose box misses the tile skipped, edges through LDS in chunks),
//                     roi_row_kernel + roi_col_kernel (the separable dilation: horizontal distance per pixel, then dx^2 + dv^2 <= r^2).
//
// The rasters of all logs live in ONE uint8 buffer (the atlas) described by a table of rvRoiLayer records; every sweep names its layer,
// so one launch serves a batch whose sweeps come from different logs.  fp64 without fused multiply-add contraction (the pragma): the
// cell a coordinate lands in has to equal NumPy's bit for bit.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int TILE_W = 64, TILE_H = 4;  // pixels of one fill workgroup: one wave per image row segment
constexpr int EDGE_CHUNK = 256;         // edges staged per pass: 8 KB of LDS

struct RoiArgs {
    const int32_t* layer_index;  // (n_sweeps)
    const double* pose;          // (n_sweeps, 12): city_SE3_ego, row-major 3 x 4
    const uint8_t* raster;
    const rvRoiLayer* layers;
    int64_t raster_bytes;
    int n_sweeps, n_layers;
    unsigned long long* stray;
};

// the declared lookup of an ego-frame point (x, y, z) of sweep b (0 <= b < n_sweeps)
__device__ __forceinline__ uint8_t roi_lookup(const RoiArgs& a, int b, double x, double y, double z) {
    const int layer = a.layer_index[b];
    if (layer < 0 || layer >= a.n_layers) return 0;
    const rvRoiLayer L = a.layers[layer];
    const double* T = a.pose + (int64_t)b * 12;
    const double cx = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    const double cy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    const double ra = (cx + L.tx) * L.s, rb = (cy + L.ty) * L.s;
    // truncation toward zero: (-1, 0) lands in cell 0; the comparisons are false for NaN and keep the casts in range
    if (!(ra > -1.0 && ra < (double)L.width && rb > -1.0 && rb < (double)L.height)) return 0;
    const int64_t u = (int64_t)ra, v = (int64_t)rb;
    const int64_t at = L.offset + v * (int64_t)L.width + u;
    if (at < 0 || at >= a.raster_bytes) return 0;  // (rv_roi_atlas_check rejects such a table; never read past the buffer)
    return a.raster[at] != 0 ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void roi_points_kernel(const RoiArgs a, const T* xyz, const int64_t* off, int64_t n, uint8_t* out) {
    const int64_t first = off[0], last = off[a.n_sweeps];
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        if (i < first || i >= last) {
            out[i] = 0;
            atomicAdd(a.stray, 1ull);
            continue;
        }
        int lo = 0, hi = a.n_sweeps;  // the last sweep whose offset is <= i (empty sweeps in front of it are passed over)
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (off[mid] <= i) lo = mid;
            else hi = mid;
        }
        out[i] = roi_lookup(a, lo, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]);
    }
}

__global__ __launch_bounds__(THREADS) void roi_boxes_kernel(const RoiArgs a, const float* boxes, const int64_t* batch_index, int64_t n, uint8_t* out) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t b = batch_index[i];
    if (b < 0 || b >= a.n_sweeps) {
        out[i] = 0;
        atomicAdd(a.stray, 1ull);
        return;
    }
    const float* r = boxes + i * 10;
    const double cx = r[0], cy = r[1], cz = r[2];
    const double hl = 0.5 * (double)r[3], hw = 0.5 * (double)r[4], hh = 0.5 * (double)r[5];
    const double qw = r[6], qx = r[7], qy = r[8], qz = r[9];
    const double R[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw),       2.0 * (qx * qz + qy * qw),
                         2.0 * (qx * qy + qz * qw),       1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw),
                         2.0 * (qx * qz - qy * qw),       2.0 * (qy * qz + qx * qw),       1.0 - 2.0 * (qx * qx + qy * qy)};
    uint8_t inside = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double dx = (k & 4) ? -hl : hl, dy = (k & 2) ? -hw : hw, dz = (k & 1) ? -hh : hh;
        const double vx = cx + ((R[0] * dx + R[1] * dy) + R[2] * dz);
        const double vy = cy + ((R[3] * dx + R[4] * dy) + R[5] * dz);
        const double vz = cz + ((R[6] * dx + R[7] * dy) + R[8] * dz);
        inside |= roi_lookup(a, (int)b, vx, vy, vz);
    }
    out[i] = inside;
}

// ---------------------------------------------------------------------------------------
// raster builder
// ---------------------------------------------------------------------------------------
struct RasterArgs {
    const double* vertices;      // (n_vertices, 2) city frame
    const int64_t* poly_off;     // (n_polys + 1)
    int64_t n_vertices;
    int n_polys, height, width, reach;  // reach = min(floor(r), max(height, width)): the largest offset that can matter
    double s, tx, ty, r2;
    double* bbox;      // workspace (n_polys, 4): min x, max x, min y, max y in raster coordinates
    int32_t* dist;     // workspace (height, width): horizontal distance to the nearest drivable pixel, reach + 1 = none
    uint8_t* drivable; // (height, width)
    uint8_t* roi;      // (height, width)
};

__device__ __forceinline__ int64_t clamp_off(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(THREADS) void roi_bbox_kernel(const RasterArgs a) {
    __shared__ double part[4][THREADS / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int64_t v0 = clamp_off(a.poly_off[p], 0, a.n_vertices), v1 = clamp_off(a.poly_off[p + 1], v0, a.n_vertices);
    double m[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (int64_t i = v0 + tid; i < v1; i += THREADS) {
        const double x = (a.vertices[2 * i] + a.tx) * a.s, y = (a.vertices[2 * i + 1] + a.ty) * a.s;
        m[0] = fmin(m[0], x), m[1] = fmax(m[1], x), m[2] = fmin(m[2], y), m[3] = fmax(m[3], y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m[0] = fmin(m[0], __shfl_xor(m[0], o, 64)), m[1] = fmax(m[1], __shfl_xor(m[1], o, 64));
        m[2] = fmin(m[2], __shfl_xor(m[2], o, 64)), m[3] = fmax(m[3], __shfl_xor(m[3], o, 64));
    }
    if ((tid & 63) == 0)
        for (int k = 0; k < 4; ++k) part[k][tid >> 6] = m[k];
    __syncthreads();
    if (tid < 4) {
        double v = part[tid][0];
        for (int w = 1; w < THREADS / 64; ++w) v = (tid & 1) ? fmax(v, part[tid][w]) : fmin(v, part[tid][w]);
        a.bbox[p * 4 + tid] = v;
    }
}

__global__ __launch_bounds__(THREADS) void roi_fill_kernel(const RasterArgs a) {
    __shared__ double edge[EDGE_CHUNK][4];  // a.x, a.y, b.x, b.y in raster coordinates
    const int tid = threadIdx.x;
    const int u0 = blockIdx.x * TILE_W, v0 = blockIdx.y * TILE_H;
    const int u = u0 + (tid & (TILE_W - 1)), v = v0 + tid / TILE_W;
    const double cx = (double)u + 0.5, cy = (double)v + 0.5;
    // pixel centres of the tile (the part beyond the image edge included: the skip only has to be conservative)
    const double tx0 = (double)u0 + 0.5, ty0 = (double)v0 + 0.5, ty1 = (double)(v0 + TILE_H - 1) + 0.5;
    bool inside = false;
    for (int p = 0; p < a.n_polys; ++p) {
        const double* bb = a.bbox + p * 4;
        // an edge counts only where min y <= cy < max y (exact) and its crossing lies right of cx: the crossing is within rounding of
        // [min x, max x], so one whole pixel of slack keeps the skip exact.  The condition is the same for the whole workgroup.
        if (!(ty1 >= bb[2] && ty0 < bb[3] && tx0 <= bb[1] + 1.0)) continue;
        const int64_t p0 = clamp_off(a.poly_off[p], 0, a.n_vertices), p1 = clamp_off(a.poly_off[p + 1], p0, a.n_vertices);
        const int64_t n = p1 - p0;
        int crossings = 0;
        for (int64_t e0 = 0; e0 < n; e0 += EDGE_CHUNK) {
            const int n_e = (int)(n - e0 < EDGE_CHUNK ? n - e0 : EDGE_CHUNK);
            __syncthreads();
            for (int j = tid; j < n_e; j += THREADS) {
                const int64_t i = p0 + e0 + j, k = e0 + j + 1 < n ? i + 1 : p0;  // the last vertex closes onto the first
                edge[j][0] = (a.vertices[2 * i] + a.tx) * a.s, edge[j][1] = (a.vertices[2 * i + 1] + a.ty) * a.s;
                edge[j][2] = (a.vertices[2 * k] + a.tx) * a.s, edge[j][3] = (a.vertices[2 * k + 1] + a.ty) * a.s;
            }
            __syncthreads();
            for (int j = 0; j < n_e; ++j) {  // (every lane reads the same LDS words: broadcast)
                const double ax = edge[j][0], ay = edge[j][1], bx = edge[j][2], by = edge[j][3];
                if ((ay <= cy) != (by <= cy) && ax + (cy - ay) * (bx - ax) / (by - ay) > cx) ++crossings;
            }
        }
        inside = inside || (crossings & 1);
    }
    if (u < a.width && v < a.height) a.drivable[(int64_t)v * a.width + u] = inside ? 1 : 0;
}

// horizontal distance to the nearest drivable pixel of the same row, reach + 1 when there is none within `reach`
__global__ __launch_bounds__(THREADS) void roi_row_kernel(const RasterArgs a) {
    const int64_t n = (int64_t)a.height * a.width;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const int u = (int)(i % a.width);
        const uint8_t* row = a.drivable + (i - u);
        int d = 0;
        for (; d <= a.reach; ++d)
            if ((u - d >= 0 && row[u - d]) || (u + d < a.width && row[u + d])) break;
        a.dist[i] = d;
    }
}

__global__ __launch_bounds__(THREADS) void roi_col_kernel(const RasterArgs a) {
    const int64_t n = (int64_t)a.height * a.width;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const int v = (int)(i / a.width);
        const int lo = v - a.reach < 0 ? -v : -a.reach, hi = v + a.reach >= a.height ? a.height - 1 - v : a.reach;
        uint8_t hit = 0;
        for (int dv = lo; dv <= hi && !hit; ++dv) {
            const int64_t dx = a.dist[i + (int64_t)dv * a.width];
            hit = dx <= a.reach && (double)(dx * dx + (int64_t)dv * dv) <= a.r2;
        }
        a.roi[i] = hit;
    }
}

int fill_args(RoiArgs& a, const char* who, int32_t n_sweeps, const int32_t* layer_index, const double* city_SE3_ego, const uint8_t* raster,
              int64_t raster_bytes, const rvRoiLayer* layers, int32_t n_layers, int64_t* stray) {
    RV_REQUIRE(n_sweeps >= 1, "%s: %d sweeps", who, n_sweeps);
    RV_REQUIRE(n_layers >= 0 && raster_bytes >= 0, "%s: %d layers, %lld raster bytes", who, n_layers, (long long)raster_bytes);
    RV_REQUIRE(layer_index && city_SE3_ego && stray, "%s: null sweep table (layer_index, city_SE3_ego, stray)", who);
    RV_REQUIRE(n_layers == 0 || (layers && (raster || raster_bytes == 0)), "%s: null atlas", who);
    RV_REQUIRE((uintptr_t)layers % 8 == 0 && (uintptr_t)city_SE3_ego % 8 == 0 && (uintptr_t)stray % 8 == 0, "%s: tables must be 8-byte aligned", who);
    a.layer_index = layer_index, a.pose = city_SE3_ego, a.raster = raster, a.layers = layers, a.raster_bytes = raster_bytes;
    a.n_sweeps = n_sweeps, a.n_layers = n_layers, a.stray = (unsigned long long*)stray;
    return 0;
}

}  // namespace

extern "C" int rv_roi_atlas_check(const rvRoiLayer* host_layers, int32_t n_layers, int64_t raster_bytes) {
    RV_REQUIRE(n_layers >= 0 && raster_bytes >= 0 && (host_layers || n_layers == 0), "rv_roi_atlas_check: %d layers, %lld raster bytes", n_layers,
               (long long)raster_bytes);
    for (int i = 0; i < n_layers; ++i) {
        const rvRoiLayer& L = host_layers[i];
        RV_REQUIRE(L.height >= 1 && L.width >= 1, "rv_roi_atlas_check: layer %d is %d x %d", i, L.height, L.width);
        RV_REQUIRE(L.offset >= 0 && L.offset <= raster_bytes && (int64_t)L.height * L.width <= raster_bytes - L.offset,
                   "rv_roi_atlas_check: layer %d (offset %lld, %d x %d) reaches beyond the %lld raster bytes", i, (long long)L.offset, L.height, L.width,
                   (long long)raster_bytes);
        RV_REQUIRE(isfinite(L.s) && L.s > 0. && isfinite(L.tx) && isfinite(L.ty), "rv_roi_atlas_check: layer %d has s = %g, t = (%g, %g)", i, L.s, L.tx,
                   L.ty);
    }
    return 0;
}

extern "C" int rv_roi_points(const void* xyz, int32_t xyz_is_f64, int64_t n, const int64_t* sweep_offsets, int32_t n_sweeps,
                             const int32_t* layer_index, const double* city_SE3_ego, const uint8_t* raster, int64_t raster_bytes,
                             const rvRoiLayer* layers, int32_t n_layers, uint8_t* within_roi, int64_t* stray, rvStream stream) {
    RoiArgs a;
    memset(&a, 0, sizeof(a));
    if (fill_args(a, "rv_roi_points", n_sweeps, layer_index, city_SE3_ego, raster, raster_bytes, layers, n_layers, stray)) return 1;
    RV_REQUIRE(n >= 0 && sweep_offsets, "rv_roi_points: n = %lld, sweep_offsets = %p", (long long)n, (const void*)sweep_offsets);
    RV_REQUIRE(n == 0 || (xyz && within_roi), "rv_roi_points: null point buffer");
    if (n == 0) return 0;
    const int64_t want = (n + THREADS - 1) / THREADS, most = (int64_t)rv_cu_count() * 8;
    const dim3 grid((unsigned)(want < most ? want : most));
    if (xyz_is_f64) hipLaunchKernelGGL(roi_points_kernel<double>, grid, dim3(THREADS), 0, (hipStream_t)stream, a, (const double*)xyz, sweep_offsets, n, within_roi);
    else hipLaunchKernelGGL(roi_points_kernel<float>, grid, dim3(THREADS), 0, (hipStream_t)stream, a, (const float*)xyz, sweep_offsets, n, within_roi);
    RV_CHECK_LAUNCH("roi_points_kernel");
    return 0;
}

extern "C" int rv_roi_boxes(const float* boxes, const int64_t* batch_index, int64_t n, int32_t n_sweeps, const int32_t* layer_index,
                            const double* city_SE3_ego, const uint8_t* raster, int64_t raster_bytes, const rvRoiLayer* layers,
                            int32_t n_layers, uint8_t* within_roi, int64_t* stray, rvStream stream) {
    RoiArgs a;
    memset(&a, 0, sizeof(a));
    if (fill_args(a, "rv_roi_boxes", n_sweeps, layer_index, city_SE3_ego, raster, raster_bytes, layers, n_layers, stray)) return 1;
    RV_REQUIRE(n >= 0 && n <= 0x7fffffffll * THREADS, "rv_roi_boxes: n = %lld", (long long)n);
    RV_REQUIRE(n == 0 || (boxes && batch_index && within_roi), "rv_roi_boxes: null box buffer");
    if (n == 0) return 0;
    hipLaunchKernelGGL(roi_boxes_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, a, boxes, batch_index, n,
                       within_roi);
    RV_CHECK_LAUNCH("roi_boxes_kernel");
    return 0;
}

extern "C" int64_t rv_roi_rasterize_workspace_bytes(int32_t n_polygons, int32_t height, int32_t width) {
    if (n_polygons < 0 || height < 1 || width < 1) return 0;
    return rv_align256((int64_t)(n_polygons > 0 ? n_polygons : 1) * 4 * (int64_t)sizeof(double)) + rv_align256((int64_t)height * width * (int64_t)sizeof(int32_t));
}

extern "C" int rv_roi_rasterize(const double* vertices, const int64_t* polygon_offsets, int64_t n_vertices, int32_t n_polygons, double s, double tx,
                                double ty, int32_t height, int32_t width, double r, void* workspace, uint8_t* drivable, uint8_t* roi,
                                rvStream stream) {
    RV_REQUIRE(n_vertices >= 0 && n_polygons >= 0 && polygon_offsets, "rv_roi_rasterize: %lld vertices, %d polygons", (long long)n_vertices, n_polygons);
    RV_REQUIRE(n_vertices == 0 || vertices, "rv_roi_rasterize: null vertices");
    RV_REQUIRE(height >= 1 && width >= 1 && (int64_t)height * width <= 0x7fffffff, "rv_roi_rasterize: a raster of %d x %d", height, width);
    RV_REQUIRE(isfinite(s) && s > 0. && isfinite(tx) && isfinite(ty), "rv_roi_rasterize: s = %g, t = (%g, %g)", s, tx, ty);
    RV_REQUIRE(isfinite(r) && r >= 0., "rv_roi_rasterize: a dilation radius of %g pixels", r);
    RV_REQUIRE(workspace && drivable && roi, "rv_roi_rasterize: null output or workspace");
    RV_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)vertices % 8 == 0, "rv_roi_rasterize: vertices and workspace must be 8-byte aligned");
    RasterArgs a;
    memset(&a, 0, sizeof(a));
    a.vertices = vertices, a.poly_off = polygon_offsets, a.n_vertices = n_vertices, a.n_polys = n_polygons, a.height = height, a.width = width;
    const int longest = height > width ? height : width;
    a.reach = r < (double)longest ? (int)floor(r) : longest;
    a.s = s, a.tx = tx, a.ty = ty, a.r2 = r * r;
    char* ws = (char*)workspace;
    a.bbox = (double*)ws;
    ws += rv_align256((int64_t)(n_polygons > 0 ? n_polygons : 1) * 4 * (int64_t)sizeof(double));
    a.dist = (int32_t*)ws;
    a.drivable = drivable, a.roi = roi;
    hipStream_t st = (hipStream_t)stream;
    if (n_polygons > 0) hipLaunchKernelGGL(roi_bbox_kernel, dim3((unsigned)n_polygons), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(roi_fill_kernel, dim3((unsigned)((width + TILE_W - 1) / TILE_W), (unsigned)((height + TILE_H - 1) / TILE_H)), dim3(THREADS), 0, st, a);
    const int64_t want = ((int64_t)height * width + THREADS - 1) / THREADS, most = (int64_t)rv_cu_count() * 8;
    const dim3 grid((unsigned)(want < most ? want : most));
    hipLaunchKernelGGL(roi_row_kernel, grid, dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(roi_col_kernel, grid, dim3(THREADS), 0, st, a);
    RV_CHECK_LAUNCH("roi raster kernels");
    return 0;
}
