// targets.hip -- dense target assignment on device (no per-instance host loop, no host syncs).
//
// Reference: compute_targets (nn/heads/detection_head.py:496-665) with cuboids_to_vertices /
// compute_interior_points_mask (math/polytope.py:14-107) and encode_regression_targets
// (detection_head.py:460-493), for the layout the rv-* configs use (one stride-1 FPN level, one
// task).  Numerics follow the reference: box vertices in fp32 through the yaw-only quaternion,
// the three slab tests in fp64, the centre offset / azimuth rotation in fp32, log / sin / cos of
// the box parameters in fp64 rounded to fp32.
//
//   pass 1  per (pixel, box of the pixel's sweep): inside test -> per-box interior-point counts
//           (wave ballot + one atomicAdd per wave and box)
//   pass 2  per sweep: rank boxes by (count ascending, original order) == the reference's stable sort
//   pass 3  per pixel: the containing box of smallest rank wins -> label, panoptic id (rank+1),
//           points_per_obj, regression targets; marks the box as owning a pixel
//   pass 4  num_objects = number of boxes that own >= 1 pixel (== sum over sweeps of the distinct
//           non-background panoptic ids, detection_head.py:379-390)
// These four passes serve rv_assign_targets (one stride-1 level, one task).  Several levels and tasks: the ml_* kernels further down
// (rv_assign_targets_multilevel), which run the slab tests once per full-resolution pixel for all levels.
#include "common.h"
#include "cuboid_interior.h"

namespace {

constexpr int kBoxTile = 64;

template <bool ASSIGN>
__global__ __launch_bounds__(256) void box_pixel_kernel(const double* cuboids, const int32_t* box_offsets, const float* cart,
                                                        int H, int W, int n_cls, int az_inv, int32_t* counts,
                                                        const int32_t* rank, int32_t* owned, int64_t* labels,
                                                        int64_t* panoptics, float* reg, int64_t* ppo) {
    __shared__ BoxPlanes planes[kBoxTile];
    const int b = blockIdx.y;
    const int64_t hw = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = pix < hw;
    const float* c0 = cart + (int64_t)b * 3 * hw;
    const float pxf = valid ? c0[pix] : 0.f, pyf = valid ? c0[hw + pix] : 0.f, pzf = valid ? c0[2 * hw + pix] : 0.f;
    const double px = pxf, py = pyf, pz = pzf;
    const int m0 = box_offsets[b], m1 = box_offsets[b + 1];
    int best_rank = 0x7fffffff, best_box = -1;
    for (int t0 = m0; t0 < m1; t0 += kBoxTile) {
        const int nt = (m1 - t0) < kBoxTile ? (m1 - t0) : kBoxTile;
        __syncthreads();
        if ((int)threadIdx.x < nt) make_planes(cuboids + (int64_t)(t0 + threadIdx.x) * 10, &planes[threadIdx.x]);
        __syncthreads();
        for (int k = 0; k < nt; ++k) {
            const bool in = valid && inside(planes[k], px, py, pz);
            if (!ASSIGN) {
                const unsigned long long bal = __ballot(in);
                if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&counts[t0 + k], __popcll(bal));
            } else if (in) {
                const int r = rank[t0 + k];
                if (r < best_rank) {
                    best_rank = r;
                    best_box = t0 + k;
                }
            }
        }
    }
    if (!ASSIGN || !valid) return;
    const int64_t o = (int64_t)b * hw + pix;
    if (best_box < 0) {
        labels[o] = n_cls;
        panoptics[o] = 0;
        ppo[o] = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) reg[((int64_t)b * 8 + j) * hw + pix] = 0.f;
        return;
    }
    const double* cub = cuboids + (int64_t)best_box * 10;
    labels[o] = (int64_t)cub[8];
    panoptics[o] = best_rank + 1;
    ppo[o] = counts[best_box];
    owned[best_box] = 1;
    float ox = (float)cub[0] - pxf, oy = (float)cub[1] - pyf;
    const float oz = (float)cub[2] - pzf;
    double rots = cub[6];
    if (az_inv) {
        const float az = atan2f(pyf, pxf);
        rots -= (double)az;
        const float c = cosf(az), s = sinf(az);
        const float x1 = c * ox + s * oy, x2 = -s * ox + c * oy;
        ox = x1;
        oy = x2;
    }
    float* r = reg + (int64_t)b * 8 * hw + pix;
    r[0] = ox;
    r[hw] = oy;
    r[2 * hw] = oz;
    r[3 * hw] = (float)log(cub[3]);
    r[4 * hw] = (float)log(cub[4]);
    r[5 * hw] = (float)log(cub[5]);
    r[6 * hw] = (float)sin(rots);
    r[7 * hw] = (float)cos(rots);
}

__global__ void rank_kernel(const int32_t* box_offsets, const int32_t* counts, int32_t* rank) {
    const int b = blockIdx.x;
    const int m0 = box_offsets[b], m1 = box_offsets[b + 1];
    for (int i = m0 + threadIdx.x; i < m1; i += blockDim.x) {
        const int ci = counts[i];
        int r = 0;
        for (int j = m0; j < m1; ++j) {
            const int cj = counts[j];
            r += (cj < ci) || (cj == ci && j < i);
        }
        rank[i] = r;
    }
}

__global__ void count_owned_kernel(const int32_t* owned, int m, int32_t* num_objects) {
    int s = 0;
    for (int i = threadIdx.x; i < m; i += blockDim.x) s += owned[i] != 0;
    s = (int)wave_sum((float)s);
    __shared__ int part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *num_objects = part[0] + part[1] + part[2] + part[3];
}

// ---- several levels x several tasks (compute_targets, detection_head.py:496-665, with its loops over strides and tasks) ----
//   pass 1  per (FULL-RESOLUTION pixel, box of the sweep): ONE inside test; a hit counts for every level whose stride divides the
//           pixel's column (wave ballot per level, one atomicAdd per wave, box and level with a hit)
//   pass 2  per (sweep, level): rank the boxes that pass the level's range filter among those of their own task by the STRIDED count
//   pass 3  per full-resolution pixel: the inside tests once more; per (level that sees the pixel, task) the containing box of
//           smallest rank, kept in LDS (a register array indexed by a run-time slot would live in scratch memory)
//   pass 4  per (level, task): boxes that own >= 1 pixel
// label, panoptic id, points_per_obj and the encoded regression targets (encode_regression_targets, detection_head.py:460-493) of one
// pixel whose owner is `best_box` (< 0: background); `pix` indexes the (H, W') plane of `hw` pixels the outputs are laid out on.
// The arithmetic of box_pixel_kernel<true>'s tail, which stays as it is: the one-level entry point keeps its machine code.
__device__ __forceinline__ void write_pixel_targets(const double* cuboids, int best_box, int best_rank, int count, int n_cls, int az_inv,
                                                    float pxf, float pyf, float pzf, int b, int64_t hw, int64_t pix, int64_t* labels,
                                                    int64_t* panoptics, float* reg, int64_t* ppo) {
    const int64_t o = (int64_t)b * hw + pix;
    if (best_box < 0) {
        labels[o] = n_cls;
        panoptics[o] = 0;
        ppo[o] = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) reg[((int64_t)b * 8 + j) * hw + pix] = 0.f;
        return;
    }
    const double* cub = cuboids + (int64_t)best_box * 10;
    labels[o] = (int64_t)cub[8];
    panoptics[o] = best_rank + 1;
    ppo[o] = count;
    float ox = (float)cub[0] - pxf, oy = (float)cub[1] - pyf;
    const float oz = (float)cub[2] - pzf;
    double rots = cub[6];
    if (az_inv) {
        const float az = atan2f(pyf, pxf);
        rots -= (double)az;
        const float c = cosf(az), s = sinf(az);
        const float x1 = c * ox + s * oy, x2 = -s * ox + c * oy;
        ox = x1;
        oy = x2;
    }
    float* r = reg + (int64_t)b * 8 * hw + pix;
    r[0] = ox;
    r[hw] = oy;
    r[2 * hw] = oz;
    r[3 * hw] = (float)log(cub[3]);
    r[4 * hw] = (float)log(cub[4]);
    r[5 * hw] = (float)log(cub[5]);
    r[6 * hw] = (float)sin(rots);
    r[7 * hw] = (float)cos(rots);
}

struct MlTable {
    int n_levels, n_tasks;
    int stride[RV_ML_MAX_LEVELS], use_range[RV_ML_MAX_LEVELS];
    double lower[RV_ML_MAX_LEVELS], upper[RV_ML_MAX_LEVELS];
    int task_id[RV_ML_MAX_ENTRIES], task_cls[RV_ML_MAX_ENTRIES];
    rvTargetOut out[RV_ML_MAX_ENTRIES];
};

// bit l set: the annotation belongs to level l (:568-582; fp64 like the reference's annotation table)
__device__ __forceinline__ unsigned box_levels(const MlTable& t, const double* cub) {
    const double d = sqrt(cub[0] * cub[0] + cub[1] * cub[1] + cub[2] * cub[2]);
    unsigned bits = 0;
    for (int l = 0; l < t.n_levels; ++l)
        if (!t.use_range[l] || (d > t.lower[l] && d <= t.upper[l])) bits |= 1u << l;
    return bits;
}

__device__ __forceinline__ int box_task(const MlTable& t, const double* cub) {
    const int id = (int)cub[7];
    for (int k = 0; k < t.n_tasks; ++k)
        if (t.task_id[k] == id) return k;
    return -1;
}

__device__ __forceinline__ unsigned pixel_levels(const MlTable& t, int col) {
    unsigned bits = 0;
    for (int l = 0; l < t.n_levels; ++l)
        if (col % t.stride[l] == 0) bits |= 1u << l;
    return bits;
}

__global__ __launch_bounds__(256) void ml_count_kernel(const MlTable t, const double* cuboids, int m, const int32_t* box_offsets,
                                                       const float* cart, int H, int W, int32_t* counts) {
    __shared__ BoxPlanes planes[kBoxTile];
    const int b = blockIdx.y;
    const int64_t hw = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = pix < hw;
    const float* c0 = cart + (int64_t)b * 3 * hw;
    const double px = valid ? c0[pix] : 0.f, py = valid ? c0[hw + pix] : 0.f, pz = valid ? c0[2 * hw + pix] : 0.f;
    const unsigned lv = valid ? pixel_levels(t, (int)(pix % W)) : 0u;
    const int m0 = box_offsets[b], m1 = box_offsets[b + 1];
    for (int t0 = m0; t0 < m1; t0 += kBoxTile) {
        const int nt = (m1 - t0) < kBoxTile ? (m1 - t0) : kBoxTile;
        __syncthreads();
        if ((int)threadIdx.x < nt) make_planes(cuboids + (int64_t)(t0 + threadIdx.x) * 10, &planes[threadIdx.x]);
        __syncthreads();
        for (int k = 0; k < nt; ++k) {
            const bool in = valid && inside(planes[k], px, py, pz);
            if (!__ballot(in)) continue;  // (wave-uniform: most waves see no box at all)
            for (int l = 0; l < t.n_levels; ++l) {
                const unsigned long long bal = __ballot(in && ((lv >> l) & 1u));
                if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&counts[(int64_t)l * m + t0 + k], __popcll(bal));
            }
        }
    }
}

__global__ void ml_rank_kernel(const MlTable t, const double* cuboids, int m, const int32_t* box_offsets, const int32_t* counts,
                               int32_t* rank) {
    const int b = blockIdx.x, l = blockIdx.y;
    const int m0 = box_offsets[b], m1 = box_offsets[b + 1];
    const int32_t* cnt = counts + (int64_t)l * m;
    for (int i = m0 + threadIdx.x; i < m1; i += blockDim.x) {
        const double* ci = cuboids + (int64_t)i * 10;
        const int ti = box_task(t, ci);
        int r = 0x7fffffff;  // (not of this level or of no task: never wins a pixel)
        if (ti >= 0 && ((box_levels(t, ci) >> l) & 1u)) {
            r = 0;
            for (int j = m0; j < m1; ++j) {
                const double* cj = cuboids + (int64_t)j * 10;
                if (box_task(t, cj) != ti || !((box_levels(t, cj) >> l) & 1u)) continue;
                r += (cnt[j] < cnt[i]) || (cnt[j] == cnt[i] && j < i);
            }
        }
        rank[(int64_t)l * m + i] = r;
    }
}

__global__ __launch_bounds__(256) void ml_assign_kernel(const MlTable t, const double* cuboids, int m, const int32_t* box_offsets,
                                                        const float* cart, int H, int W, int az_inv, const int32_t* counts,
                                                        const int32_t* rank, int32_t* owned) {
    __shared__ BoxPlanes planes[kBoxTile];
    __shared__ int tile_task[kBoxTile];
    __shared__ int best_rank[RV_ML_MAX_ENTRIES][256], best_box[RV_ML_MAX_ENTRIES][256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t hw = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * 256 + tid;
    const bool valid = pix < hw;
    const float* c0 = cart + (int64_t)b * 3 * hw;
    const float pxf = valid ? c0[pix] : 0.f, pyf = valid ? c0[hw + pix] : 0.f, pzf = valid ? c0[2 * hw + pix] : 0.f;
    const double px = pxf, py = pyf, pz = pzf;
    const int col = (int)(pix % W), row = (int)(pix / W);
    const unsigned lv = valid ? pixel_levels(t, col) : 0u;
    const int n_entries = t.n_levels * t.n_tasks;
    for (int e = 0; e < n_entries; ++e) {
        best_rank[e][tid] = 0x7fffffff;
        best_box[e][tid] = -1;
    }
    const int m0 = m > 0 ? box_offsets[b] : 0, m1 = m > 0 ? box_offsets[b + 1] : 0;
    for (int t0 = m0; t0 < m1; t0 += kBoxTile) {
        const int nt = (m1 - t0) < kBoxTile ? (m1 - t0) : kBoxTile;
        __syncthreads();
        if (tid < nt) {
            make_planes(cuboids + (int64_t)(t0 + tid) * 10, &planes[tid]);
            tile_task[tid] = box_task(t, cuboids + (int64_t)(t0 + tid) * 10);
        }
        __syncthreads();
        for (int k = 0; k < nt; ++k) {
            if (!(valid && inside(planes[k], px, py, pz)) || tile_task[k] < 0) continue;
            for (int l = 0; l < t.n_levels; ++l) {
                if (!((lv >> l) & 1u)) continue;
                const int r = rank[(int64_t)l * m + t0 + k];  // (0x7fffffff when the box is not of level l)
                const int e = l * t.n_tasks + tile_task[k];
                if (r < best_rank[e][tid]) {
                    best_rank[e][tid] = r;
                    best_box[e][tid] = t0 + k;
                }
            }
        }
    }
    if (!valid) return;
    for (int l = 0; l < t.n_levels; ++l) {
        if (!((lv >> l) & 1u)) continue;
        const int ws = W / t.stride[l];
        const int64_t hws = (int64_t)H * ws, spix = (int64_t)row * ws + col / t.stride[l];
        for (int k = 0; k < t.n_tasks; ++k) {
            const int e = l * t.n_tasks + k;
            const int bb = best_box[e][tid];
            if (bb >= 0) owned[(int64_t)l * m + bb] = 1;
            const rvTargetOut& o = t.out[e];
            write_pixel_targets(cuboids, bb, best_rank[e][tid], bb >= 0 ? counts[(int64_t)l * m + bb] : 0, t.task_cls[k], az_inv, pxf, pyf,
                                pzf, b, hws, spix, o.labels, o.panoptics, o.reg_targets, o.points_per_obj);
        }
    }
}

__global__ void ml_count_owned_kernel(const MlTable t, const double* cuboids, int m, const int32_t* owned, int32_t* num_objects) {
    const int e = blockIdx.x, l = e / t.n_tasks, k = e % t.n_tasks;
    int s = 0;
    for (int i = threadIdx.x; i < m; i += blockDim.x) s += owned[(int64_t)l * m + i] != 0 && box_task(t, cuboids + (int64_t)i * 10) == k;
    s = (int)wave_sum((float)s);
    __shared__ int part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) num_objects[e] = part[0] + part[1] + part[2] + part[3];
}

}  // namespace

extern "C" int rv_assign_targets(const double* cuboids, int32_t m, const int32_t* box_offsets, const float* cart, int32_t B,
                                 int32_t H, int32_t W, int32_t n_cls, int32_t azimuth_invariant, int32_t* counts,
                                 int32_t* order, int32_t* owned, int64_t* labels, int64_t* panoptics, float* reg_targets,
                                 int64_t* points_per_obj, int32_t* num_objects, rvStream stream) {
    RV_REQUIRE(box_offsets && cart && labels && panoptics && reg_targets && points_per_obj && num_objects, "rv_assign_targets: null argument");
    RV_REQUIRE(m == 0 || (cuboids && counts && order && owned), "rv_assign_targets: null box buffers");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(num_objects, 0, sizeof(int32_t), st);
    if (m > 0 && e == hipSuccess) e = hipMemsetAsync(counts, 0, sizeof(int32_t) * m, st);
    if (m > 0 && e == hipSuccess) e = hipMemsetAsync(owned, 0, sizeof(int32_t) * m, st);
    if (e != hipSuccess) RV_FAIL("rv_assign_targets: %s", hipGetErrorString(e));
    const dim3 grid(rv_ceil_div((int64_t)H * W, 256), B);
    if (m > 0) {
        hipLaunchKernelGGL(box_pixel_kernel<false>, grid, dim3(256), 0, st, cuboids, box_offsets, cart, H, W, n_cls,
                           azimuth_invariant, counts, (const int32_t*)nullptr, owned, labels, panoptics, reg_targets,
                           points_per_obj);
        hipLaunchKernelGGL(rank_kernel, dim3(B), dim3(128), 0, st, box_offsets, counts, order);
    }
    hipLaunchKernelGGL(box_pixel_kernel<true>, grid, dim3(256), 0, st, cuboids, box_offsets, cart, H, W, n_cls,
                       azimuth_invariant, counts, (const int32_t*)order, owned, labels, panoptics, reg_targets, points_per_obj);
    if (m > 0) hipLaunchKernelGGL(count_owned_kernel, dim3(1), dim3(256), 0, st, owned, m, num_objects);
    RV_CHECK_LAUNCH("rv_assign_targets kernels");
    return 0;
}

extern "C" int rv_assign_targets_multilevel(const double* cuboids, int32_t m, const int32_t* box_offsets, const float* cart, int32_t B,
                                            int32_t H, int32_t W, int32_t n_levels, const rvTargetLevel* host_levels, int32_t n_tasks,
                                            const int32_t* host_task_ids, const int32_t* host_task_classes, int32_t azimuth_invariant,
                                            int32_t* scratch, const rvTargetOut* host_outs, int32_t* num_objects, rvStream stream) {
    RV_REQUIRE(box_offsets && cart && host_levels && host_task_ids && host_task_classes && host_outs && num_objects,
               "rv_assign_targets_multilevel: null argument");
    RV_REQUIRE(m == 0 || (cuboids && scratch), "rv_assign_targets_multilevel: null box buffers");
    RV_REQUIRE(B > 0 && H > 0 && W > 0 && m >= 0, "rv_assign_targets_multilevel: bad shape");
    RV_REQUIRE(n_levels >= 1 && n_levels <= RV_ML_MAX_LEVELS && n_tasks >= 1 && n_levels * n_tasks <= RV_ML_MAX_ENTRIES,
               "rv_assign_targets_multilevel: %d levels x %d tasks (at most %d levels, %d entries)", n_levels, n_tasks, RV_ML_MAX_LEVELS,
               RV_ML_MAX_ENTRIES);
    MlTable t;
    memset(&t, 0, sizeof(t));
    t.n_levels = n_levels;
    t.n_tasks = n_tasks;
    for (int l = 0; l < n_levels; ++l) {
        RV_REQUIRE(host_levels[l].stride >= 1 && W % host_levels[l].stride == 0, "rv_assign_targets_multilevel: stride %d does not divide W = %d",
                   host_levels[l].stride, W);
        t.stride[l] = host_levels[l].stride;
        t.use_range[l] = host_levels[l].use_range;
        t.lower[l] = host_levels[l].lower;
        t.upper[l] = host_levels[l].upper;
    }
    for (int k = 0; k < n_tasks; ++k) {
        t.task_id[k] = host_task_ids[k];
        t.task_cls[k] = host_task_classes[k];
    }
    for (int e = 0; e < n_levels * n_tasks; ++e) {
        RV_REQUIRE(host_outs[e].labels && host_outs[e].panoptics && host_outs[e].reg_targets && host_outs[e].points_per_obj,
                   "rv_assign_targets_multilevel: null output of entry %d", e);
        t.out[e] = host_outs[e];
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t lm = (int64_t)n_levels * m;
    int32_t *counts = scratch, *rank = scratch + lm, *owned = scratch + 2 * lm;
    hipError_t e = hipMemsetAsync(num_objects, 0, sizeof(int32_t) * n_levels * n_tasks, st);
    if (m > 0 && e == hipSuccess) e = hipMemsetAsync(counts, 0, sizeof(int32_t) * lm, st);
    if (m > 0 && e == hipSuccess) e = hipMemsetAsync(owned, 0, sizeof(int32_t) * lm, st);
    if (e != hipSuccess) RV_FAIL("rv_assign_targets_multilevel: %s", hipGetErrorString(e));
    const dim3 grid(rv_ceil_div((int64_t)H * W, 256), B);
    if (m > 0) {
        hipLaunchKernelGGL(ml_count_kernel, grid, dim3(256), 0, st, t, cuboids, m, box_offsets, cart, H, W, counts);
        hipLaunchKernelGGL(ml_rank_kernel, dim3(B, n_levels), dim3(128), 0, st, t, cuboids, m, box_offsets, (const int32_t*)counts, rank);
    }
    hipLaunchKernelGGL(ml_assign_kernel, grid, dim3(256), 0, st, t, cuboids, m, box_offsets, cart, H, W, azimuth_invariant,
                       (const int32_t*)counts, (const int32_t*)rank, owned);
    if (m > 0)
        hipLaunchKernelGGL(ml_count_owned_kernel, dim3(n_levels * n_tasks), dim3(256), 0, st, t, cuboids, m, (const int32_t*)owned, num_objects);
    RV_CHECK_LAUNCH("rv_assign_targets_multilevel kernels");
    return 0;
}
