// dbsample.hip -- object-database sampling ("GT paste") and the mid-chain point_dropout of the loader, on device.
//
// Reference: sample_database (prototype/loader.py:708-789), called from DataLoader.__getitem__ (:672-682) after the augmentations
// and before subsample_range_view, i.e. on the UNPADDED image; _point_dropout (:506-512) inside apply_augmentations (:514-549).
//
// The object database sits in HBM as one CSR block (prototype/database.py, uploaded once): points (P, 3 + F) fp32 = x, y, z and the
// feature columns, range (P) fp32, index (P) int32 = flat pixel h * W + w of the unpadded image, offsets (N_obj + 1) int64.
//
// Paste of a batch (steps 4-6 of the reference: concat in sample order, sort by range, unique("index", keep="first"), scatter,
// `range_view *= range_mask`), three launches whatever the number of samples:
//   1  db_prepare_kernel   keys := all ones, owned := 0, work list = exclusive prefix sum of the kept samples' point counts
//   2  db_keys_kernel      one unit of work per (sweep, slot, point): atomicMin(keys[b][index], float_bits(range) << 32 | work index)
//   3  db_resolve_kernel   one pass over B * H * W pixels: a taken pixel reads its winner, every pixel leaves with features * mask
// The range is >= 0, so its bit pattern orders like its value (csrc/project.hip's z-buffer idiom).  TIE RULE: points of equal range
// that fall on one pixel go to the lower work index = the lower (slot, point) position.  The reference leaves such ties to polars'
// unstable sort; taking the first one in sample order is this library's choice, and it makes the paste deterministic.
// A pasted point always overwrites the scene's pixel: like the reference, there is no depth test against the scene.
//
// rv_db_extract is the builder's kernel (the reference ships no builder): the pixels of every annotation's cuboid, through the interior
// test of targets.hip (cuboid_interior.h), count pass - scan - fill pass, every object's pixels in ascending index order.
//
// rv_augment_dropout is rv_augment (augment.hip) with a point_dropout somewhere inside the chain.
#include "common.h"
#include "cuboid_interior.h"

namespace {

constexpr unsigned long long kNoKey = ~0ull;

// largest i in [0, n) with start[i] <= v (start ascending, start[0] <= v)
__device__ __forceinline__ int upper_slot(const int64_t* start, int n, int64_t v) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t slot_points(const int32_t* samples, const uint8_t* keep, const int64_t* offsets, int64_t n_obj, int s) {
    const int32_t obj = samples[s];
    if (!keep[s] || obj < 0 || obj >= n_obj) return 0;
    return offsets[obj + 1] - offsets[obj];
}

// keys := kNoKey (every block); owned := 0 and the work list (block 0: a 256-thread scan over the B * S slots)
__global__ __launch_bounds__(256) void db_prepare_kernel(const int32_t* samples, const uint8_t* keep, const int64_t* offsets, int64_t n_obj,
                                                         int n_slots, int64_t* slot_start, uint8_t* owned, unsigned long long* keys,
                                                         int64_t n_keys) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_keys; i += (int64_t)gridDim.x * blockDim.x) keys[i] = kNoKey;
    if (blockIdx.x != 0) return;
    __shared__ int64_t part[256];
    const int tid = threadIdx.x;
    const int per = (n_slots + 255) / 256;
    const int s0 = tid * per, s1 = (s0 + per) < n_slots ? (s0 + per) : n_slots;
    int64_t sum = 0;
    for (int s = s0; s < s1; ++s) {
        sum += slot_points(samples, keep, offsets, n_obj, s);
        owned[s] = 0;
    }
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = part[tid] - sum;  // exclusive
    for (int s = s0; s < s1; ++s) {
        slot_start[s] = run;
        run += slot_points(samples, keep, offsets, n_obj, s);
    }
    if (tid == 255) slot_start[n_slots] = part[255];
}

__global__ __launch_bounds__(256) void db_keys_kernel(const int32_t* samples, const int64_t* offsets, const float* range, const int32_t* index,
                                                      int S, int n_slots, const int64_t* slot_start, int64_t hw, unsigned long long* keys) {
    const int64_t total = slot_start[n_slots];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int s = upper_slot(slot_start, n_slots, i);
        const int64_t pt = offsets[samples[s]] + (i - slot_start[s]);
        const int64_t p = index[pt];
        if (p < 0 || p >= hw) continue;  // (the loader and the host entry refuse such a block; never store out of bounds)
        const unsigned long long key = ((unsigned long long)__float_as_uint(range[pt]) << 32) | (unsigned long long)(uint32_t)i;
        atomicMin(&keys[(int64_t)(s / S) * hw + p], key);
    }
}

template <int V>
struct Vec;
template <>
struct Vec<1> {
    typedef float f;
    typedef uint8_t m;
};
template <>
struct Vec<4> {
    typedef f32x4 f;
    typedef uint32_t m;
};

// V pixels per thread (V = 4: 16-byte accesses along W; hw % 4 == 0, so the V pixels lie in one plane of one sweep)
template <int V>
__global__ __launch_bounds__(256) void db_resolve_kernel(const float* feat_in, const float* cart_in, const uint8_t* mask_in, float* feat_out,
                                                         float* cart_out, uint8_t* mask_out, int B, int F, int64_t hw,
                                                         const unsigned long long* keys, const int32_t* samples, const int64_t* offsets,
                                                         const float* points, int n_slots, const int64_t* slot_start, uint8_t* owned) {
    typedef typename Vec<V>::f vf;
    typedef typename Vec<V>::m vm;
    const int64_t groups = (int64_t)B * hw / V;
    const int ld = 3 + F;
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = g * V;
        const int b = (int)(i / hw);
        const int64_t p = i - (int64_t)b * hw;
        unsigned long long key[V];
        const float* win[V];
        float m[V];
        uint8_t mb[V];
        const vm mv = *(const vm*)(mask_in + i);
        bool any = false;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            key[k] = keys[i + k];
            any |= key[k] != kNoKey;
            mb[k] = V == 1 ? (uint8_t)mv : (uint8_t)((uint32_t)mv >> (8 * k));
            win[k] = nullptr;
        }
        if (any) {
#pragma unroll
            for (int k = 0; k < V; ++k) {
                if (key[k] == kNoKey) continue;
                const int64_t work = (int64_t)(uint32_t)key[k];
                const int s = upper_slot(slot_start, n_slots, work);
                win[k] = points + (offsets[samples[s]] + (work - slot_start[s])) * ld;
                const float x = win[k][0], y = win[k][1], z = win[k][2];
                // np.linalg.norm of the fp32 columns > 0 (loader.py:756): unfused fp32 products and sums, as numpy forms them
                mb[k] = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z))) > 0.f ? 1 : 0;
                owned[s] = 1;  // the same value from every winner of the slot
            }
        }
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            mb[k] = mb[k] ? 1 : 0;
            m[k] = mb[k] ? 1.f : 0.f;
            packed |= (uint32_t)mb[k] << (8 * k);
        }
        *(vm*)(mask_out + i) = (vm)packed;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t o = ((int64_t)b * 3 + c) * hw + p;
            vf v = *(const vf*)(cart_in + o);
            if (any) {
                float e[V];
                __builtin_memcpy(e, &v, sizeof(v));
#pragma unroll
                for (int k = 0; k < V; ++k)
                    if (win[k]) e[k] = win[k][c];
                __builtin_memcpy(&v, e, sizeof(v));
            }
            *(vf*)(cart_out + o) = v;
        }
        for (int f = 0; f < F; ++f) {
            const int64_t o = ((int64_t)b * F + f) * hw + p;
            vf v = *(const vf*)(feat_in + o);
            float e[V];
            __builtin_memcpy(e, &v, sizeof(v));
#pragma unroll
            for (int k = 0; k < V; ++k) e[k] = (win[k] ? win[k][3 + f] : e[k]) * m[k];  // `range_view *= range_mask` over the WHOLE image (:772)
            __builtin_memcpy(&v, e, sizeof(v));
            *(vf*)(feat_out + o) = v;
        }
    }
}

// ---- builder: pixels of every annotation's cuboid ---------------------------------------------------------------------------------
// One workgroup per box walks its sweep's pixels in index order; FILL == false counts, FILL == true writes the indices at
// obj_offsets[box] + (rank of the pixel among the box's pixels): ascending index, independent of scheduling.
template <bool FILL>
__global__ __launch_bounds__(256) void db_extract_kernel(const float* cart, const uint8_t* mask, int B, int64_t hw, const double* cuboids,
                                                         const int32_t* box_offsets, int64_t* counts, const int64_t* obj_offsets,
                                                         int32_t* out_index, int64_t capacity) {
    __shared__ BoxPlanes bp;
    __shared__ int wave_n[4];
    const int box = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int b = 0;
    while (b + 1 < B && box >= box_offsets[b + 1]) ++b;
    if (tid == 0) make_planes(cuboids + (int64_t)box * 10, &bp);
    __syncthreads();
    const float* c0 = cart + (int64_t)b * 3 * hw;
    const uint8_t* m0 = mask + (int64_t)b * hw;
    int64_t base = FILL ? obj_offsets[box] : 0;
    const int64_t end = FILL ? obj_offsets[box + 1] : 0;
    for (int64_t p0 = 0; p0 < hw; p0 += 256) {
        const int64_t p = p0 + tid;
        const bool in = p < hw && m0[p] != 0 && inside(bp, (double)c0[p], (double)c0[hw + p], (double)c0[2 * hw + p]);
        const unsigned long long bal = __ballot(in);
        if (lane == 0) wave_n[wv] = __popcll(bal);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            before += k < wv ? wave_n[k] : 0;
            all += wave_n[k];
        }
        if (FILL && in) {
            const int64_t pos = base + before + __popcll(bal & ((1ull << lane) - 1ull));
            if (pos < end && pos < capacity) out_index[pos] = (int32_t)p;
        }
        base += all;
        __syncthreads();
    }
    if (!FILL && tid == 0) counts[box] = base;
}

// obj_offsets (m + 1) := exclusive prefix sum of counts (m), one workgroup
__global__ __launch_bounds__(256) void db_scan_kernel(const int64_t* counts, int m, int64_t* obj_offsets) {
    __shared__ int64_t part[256];
    const int tid = threadIdx.x;
    const int per = (m + 255) / 256;
    const int s0 = tid * per, s1 = (s0 + per) < m ? (s0 + per) : m;
    int64_t sum = 0;
    for (int s = s0; s < s1; ++s) sum += counts[s];
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = part[tid] - sum;
    for (int s = s0; s < s1; ++s) {
        obj_offsets[s] = run;
        run += counts[s];
    }
    if (tid == 255) obj_offsets[m] = part[255];
}

// ---- rv_augment with a point_dropout inside the chain ---------------------------------------------------------------------------------
struct AugParams {  // per sweep, 32 doubles (augment.hip)
    double a, b;
    double A[9];
    double t[3];
    double Ar[9];
    double tr[3];
    double use_range;
    double pad[5];
};

__global__ void augment_dropout_kernel(const float* in, float* out, int B, int C, int H, int W, int ix, int iy, int iz, int ir,
                                       const AugParams* params, const AugParams* post, const uint8_t* keep) {
    const int64_t hw = (int64_t)H * W, total = (int64_t)B * hw;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / hw);
        const int64_t p = i - b * hw;
        const int h = (int)(p / W), w = (int)(p - (int64_t)h * W);
        const AugParams& q = params[b];
        const AugParams& r = post[b];
        float* dst = out + ((int64_t)b * C) * hw + p;
        // the pixel of the dropout step's table that the steps AFTER the dropout move here
        int wd = ((int)r.a * w + (int)r.b) % W;
        if (wd < 0) wd += W;
        if (!keep[(int64_t)b * hw + (int64_t)h * W + wd]) {
            // every column was zeroed there (loader.py:506-512): later flips / rolls moved the empty pixel, later affine steps gave it
            // xyz = A_post 0 + t_post, and a later random_global_scale re-derived its range from the xyz it held by then
            for (int c = 0; c < C; ++c) {
                float v = 0.f;
                if (c == ix) v = (float)r.t[0];
                else if (c == iy) v = (float)r.t[1];
                else if (c == iz) v = (float)r.t[2];
                else if (c == ir && r.use_range != 0.0) v = (float)sqrt(r.tr[0] * r.tr[0] + r.tr[1] * r.tr[1] + r.tr[2] * r.tr[2]);
                dst[(int64_t)c * hw] = v;
            }
            continue;
        }
        int ws = ((int)q.a * w + (int)q.b) % W;
        if (ws < 0) ws += W;
        const float* src = in + ((int64_t)b * C) * hw + (int64_t)h * W + ws;
        double x = 0.0, y = 0.0, z = 0.0;
        if (ix >= 0) {
            x = (double)src[(int64_t)ix * hw];
            y = (double)src[(int64_t)iy * hw];
            z = (double)src[(int64_t)iz * hw];
        }
        for (int c = 0; c < C; ++c) {  // exactly augment_kernel's arithmetic
            float v = src[(int64_t)c * hw];
            if (c == ix) v = (float)(q.A[0] * x + q.A[1] * y + q.A[2] * z + q.t[0]);
            else if (c == iy) v = (float)(q.A[3] * x + q.A[4] * y + q.A[5] * z + q.t[1]);
            else if (c == iz) v = (float)(q.A[6] * x + q.A[7] * y + q.A[8] * z + q.t[2]);
            else if (c == ir && q.use_range != 0.0) {
                const double rx = q.Ar[0] * x + q.Ar[1] * y + q.Ar[2] * z + q.tr[0];
                const double ry = q.Ar[3] * x + q.Ar[4] * y + q.Ar[5] * z + q.tr[1];
                const double rz = q.Ar[6] * x + q.Ar[7] * y + q.Ar[8] * z + q.tr[2];
                v = (float)sqrt(rx * rx + ry * ry + rz * rz);
            }
            dst[(int64_t)c * hw] = v;
        }
    }
}

static inline unsigned grid_for(int64_t n) {
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int64_t rv_db_paste_workspace_bytes(int32_t B, int32_t S, int32_t H, int32_t W) {
    if (B <= 0 || S < 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)B * H * W * 8 + ((int64_t)B * S + 1) * 8;
}

extern "C" int rv_db_paste_keys(const int32_t* samples, const uint8_t* keep, int32_t B, int32_t S, const int64_t* offsets, int64_t n_obj,
                                const float* range, const int32_t* index, int64_t index_max, int64_t max_work, int32_t H, int32_t W,
                                uint8_t* owned, void* workspace, rvStream stream) {
    RV_REQUIRE(B > 0 && S > 0 && H > 0 && W > 0 && n_obj > 0, "rv_db_paste_keys: empty batch, sample list or database");
    RV_REQUIRE(samples && keep && offsets && range && index && owned && workspace, "rv_db_paste_keys: null argument");
    const int64_t hw = (int64_t)H * W;
    // `index_max` is the largest pixel index of the uploaded block (ObjectDatabase checks every file at load): a database made for
    // another image size must never become an out-of-range store
    RV_REQUIRE(index_max >= 0 && index_max < hw, "rv_db_paste_keys: the database holds pixel index %lld, the image has %lld pixels",
               (long long)index_max, (long long)hw);
    RV_REQUIRE(max_work >= 0 && max_work < 0xffffffffll, "rv_db_paste_keys: %lld points in one batch (the key holds a 32-bit work index)",
               (long long)max_work);
    RV_REQUIRE((int64_t)B * S < (1ll << 30), "rv_db_paste_keys: too many sample slots");
    unsigned long long* keys = (unsigned long long*)workspace;
    int64_t* slot_start = (int64_t*)(keys + (int64_t)B * hw);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(db_prepare_kernel, dim3(grid_for(B * hw)), dim3(256), 0, st, samples, keep, offsets, n_obj, B * S, slot_start, owned,
                       keys, (int64_t)B * hw);
    RV_CHECK_LAUNCH("db_prepare_kernel");
    hipLaunchKernelGGL(db_keys_kernel, dim3(grid_for(max_work)), dim3(256), 0, st, samples, offsets, range, index, S, B * S, slot_start, hw, keys);
    RV_CHECK_LAUNCH("db_keys_kernel");
    return 0;
}

extern "C" int rv_db_paste_resolve(const float* features_in, const float* cart_in, const uint8_t* mask_in, float* features_out, float* cart_out,
                                   uint8_t* mask_out, int32_t B, int32_t F, int32_t H, int32_t W, const int32_t* samples, int32_t S,
                                   const int64_t* offsets, const float* points, const void* workspace, uint8_t* owned, rvStream stream) {
    RV_REQUIRE(B > 0 && F > 0 && S > 0 && H > 0 && W > 0, "rv_db_paste_resolve: empty batch or sample list");
    RV_REQUIRE(features_in && cart_in && mask_in && features_out && cart_out && mask_out && samples && offsets && points && workspace && owned,
               "rv_db_paste_resolve: null argument");
    RV_REQUIRE(features_in != features_out && cart_in != cart_out && mask_in != mask_out, "rv_db_paste_resolve: in and out must be distinct buffers");
    const int64_t hw = (int64_t)H * W;
    const unsigned long long* keys = (const unsigned long long*)workspace;
    const int64_t* slot_start = (const int64_t*)(keys + (int64_t)B * hw);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = hw % 4 == 0 && aligned16(features_in) && aligned16(features_out) && aligned16(cart_in) && aligned16(cart_out) &&
                     aligned16(mask_in) && aligned16(mask_out);
    if (vec)
        hipLaunchKernelGGL(db_resolve_kernel<4>, dim3(grid_for(B * hw / 4)), dim3(256), 0, st, features_in, cart_in, mask_in, features_out, cart_out,
                           mask_out, B, F, hw, keys, samples, offsets, points, B * S, slot_start, owned);
    else
        hipLaunchKernelGGL(db_resolve_kernel<1>, dim3(grid_for(B * hw)), dim3(256), 0, st, features_in, cart_in, mask_in, features_out, cart_out,
                           mask_out, B, F, hw, keys, samples, offsets, points, B * S, slot_start, owned);
    RV_CHECK_LAUNCH("db_resolve_kernel");
    return 0;
}

extern "C" int rv_db_extract(const float* cart, const uint8_t* mask, int32_t B, int32_t H, int32_t W, const double* cuboids, int32_t m,
                             const int32_t* box_offsets, int64_t* counts, int64_t* obj_offsets, int32_t* out_index, int64_t capacity,
                             rvStream stream) {
    if (m == 0) return 0;
    RV_REQUIRE(B > 0 && H > 0 && W > 0 && m > 0, "rv_db_extract: empty batch");
    RV_REQUIRE((int64_t)H * W < (1ll << 31), "rv_db_extract: the pixel index must fit 32 bits");
    RV_REQUIRE(cart && mask && cuboids && box_offsets && counts && obj_offsets, "rv_db_extract: null argument");
    const int64_t hw = (int64_t)H * W;
    hipStream_t st = (hipStream_t)stream;
    if (!out_index) {  // count pass + scan
        hipLaunchKernelGGL(db_extract_kernel<false>, dim3((unsigned)m), dim3(256), 0, st, cart, mask, B, hw, cuboids, box_offsets, counts,
                           (const int64_t*)nullptr, (int32_t*)nullptr, (int64_t)0);
        RV_CHECK_LAUNCH("db_extract_kernel<count>");
        hipLaunchKernelGGL(db_scan_kernel, dim3(1), dim3(256), 0, st, counts, m, obj_offsets);
        RV_CHECK_LAUNCH("db_scan_kernel");
        return 0;
    }
    RV_REQUIRE(capacity >= 0, "rv_db_extract: negative capacity");
    hipLaunchKernelGGL(db_extract_kernel<true>, dim3((unsigned)m), dim3(256), 0, st, cart, mask, B, hw, cuboids, box_offsets, counts, obj_offsets,
                       out_index, capacity);
    RV_CHECK_LAUNCH("db_extract_kernel<fill>");
    return 0;
}

extern "C" int rv_augment_dropout(const float* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ix, int32_t iy, int32_t iz,
                                  int32_t irange, const double* params, const double* post_params, const uint8_t* keep, rvStream stream) {
    RV_REQUIRE(in && out && params && post_params && keep && in != out, "rv_augment_dropout: null or aliased argument");
    RV_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, "rv_augment_dropout: empty tensor");
    RV_REQUIRE((ix < 0 && iy < 0 && iz < 0) || (ix >= 0 && iy >= 0 && iz >= 0 && ix < C && iy < C && iz < C),
               "rv_augment_dropout: the x / y / z channel indices must be all given or all -1");
    RV_REQUIRE(irange < C && (irange < 0 || ix >= 0), "rv_augment_dropout: bad range channel");
    hipLaunchKernelGGL(augment_dropout_kernel, dim3(grid_for((int64_t)B * H * W)), dim3(256), 0, (hipStream_t)stream, in, out, B, C, H, W, ix, iy,
                       iz, irange, (const AugParams*)params, (const AugParams*)post_params, keep);
    RV_CHECK_LAUNCH("augment_dropout_kernel");
    return 0;
}
