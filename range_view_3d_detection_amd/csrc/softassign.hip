// softassign.hip -- soft target assignment with every option of `targets_config`: per-instance affinities on the device.
//
// Reference: compute_classification_targets (math/ops/assignment.py:76-147), _gaussian (:150-161), iou_2d_axis_aligned (:64-73).
// The reference loops over sweeps and instances in Python (masked_select / topk / masked_scatter_ per instance).  Here an INSTANCE is a
// slot of a table indexed by (entry, sweep, panoptic id) -- the CSR of the annotation table bounds it: n_entries * (m + B) slots --
// and every step is one launch over all pixels of all entries or one launch over all slots:
//
//   sa_affinity_kernel    per pixel with panoptics > 0: decode prediction and target, write the affinity (GAUSSIAN: exp(-d / sigma^2),
//                         BEV: clamped rotated IoU) to the entry's map; under normalize_affinities write the distance d instead and
//                         take the instance's smallest d with an unsigned atomicMin on its bit pattern (d >= 0);
//   sa_normalize_kernel   (normalize_affinities) map = exp(-(d - d_min[slot]) / sigma^2);
//   4 x { sa_hist_kernel, sa_scan_kernel }   (finite k) radix select, 8 bits per round, on the affinity's bit pattern (affinities are
//                         never negative: their bit patterns order like unsigned integers).  hist: a pixel whose high bits equal its
//                         instance's prefix adds 1 to hist[slot][digit]; scan: one wave per slot walks the 256 bins from the top, fixes
//                         the next 8 bits of the threshold and the count still to find, and zeroes the bins for the next round;
//   sa_apply_kernel       (finite k) map = map >= threshold[slot] ? map : 0.
//
// Tie rule: a pixel stays iff its affinity is >= the instance's k_actual-th largest affinity (and != 0), k_actual = min(k, |set|).
// Integer atomics and min only: the result does not depend on the order in which workgroups run.  An instance with |set| < k never
// finds its digit, keeps prefix 0 and ends with threshold 0.
//
// Compiled with -ffp-contract=off (csrc/Makefile, EXACT) for nms_geom.h: BEV affinities are bit-exact with oracle.nms.pairwise_iou on
// equal fp32 boxes.  The GAUSSIAN arithmetic below the pragma is contracted as in loss.hip, whose per-pixel affinity it restates.
#include "common.h"
#include "nms_geom.h"

namespace {

struct SaEntry {
    const float* reg;        // NHWC, ld_reg
    const float* cart;       // (B,3,H,W)
    const int64_t* pan;      // (B,H,W)
    const float* reg_targets;  // (B,8,H,W)
    float* map;              // (B,H,W)
    int ld_reg, H, W;
};

struct SaTable {
    int n, B, m;
    int block_begin[RV_ML_MAX_ENTRIES + 1];
    SaEntry e[RV_ML_MAX_ENTRIES];
    const int32_t* box_offsets;  // (B + 1), device
    uint32_t* prefix;            // per slot: the bits of the threshold fixed so far
    uint32_t* krem;              // per slot: how many values >= threshold are still to find below the prefix
    uint32_t* dmin;              // per slot: bit pattern of the smallest distance
    uint32_t* hist;              // per slot: 256 bins
    float sigma;
    int az_inv, k;
};

// slot of (entry, sweep, panoptic id) or -1: sweep b owns the slots [off[b] + b, off[b + 1] + b], one per id 0 .. count_b
__device__ __forceinline__ int64_t slot_of(const SaTable& t, int entry, int64_t b, int64_t p) {
    const int lo = t.box_offsets[b], hi = t.box_offsets[b + 1];
    // (an id beyond the sweep's box count cannot come from rv_assign_targets*: such a pixel is background; nor can a CSR beyond m)
    if (p <= 0 || p > hi - lo || lo < 0 || hi > t.m) return -1;
    return (int64_t)entry * (t.m + t.B) + lo + b + p;
}

__device__ __forceinline__ int entry_of(const SaTable& t) {
    int k = 0;
    while (k + 1 < t.n && (int)blockIdx.x >= t.block_begin[k + 1]) ++k;  // (wave-uniform: scalar loads)
    return k;
}

// BEV IoU of two boxes (x, y) / (l, w, yaw): oracle.nms.pairwise_iou on their rectangles; above the pragma, so not contracted
__device__ __forceinline__ float bev_iou(const float* cp, const float* lp, const float* cg, const float* lg) {
    float bp[5], bg[5], sp, cpn, sg, cgn;
    rect_of_box(cp[0], cp[1], lp[0], lp[1], lp[2], bp);
    rect_of_box(cg[0], cg[1], lg[0], lg[1], lg[2], bg);
    yaw_sincos(lp[2], sp, cpn);
    yaw_sincos(lg[2], sg, cgn);
    return rotated_iou(bp, sp, cpn, bg, sg, cgn);
}

#pragma clang fp contract(fast)

// centre of decode_range_view: fp64 arithmetic rounded to fp32 (math/ops/coding.py:126-144) -- loss.hip's decode_centre
__device__ __forceinline__ void decode_centre(const float* r, float px, float py, float pz, int az_inv, float* c) {
    double dx = r[0], dy = r[1];
    if (az_inv) {
        const double az = atan2((double)py, (double)px);
        const double s = sin(az), co = cos(az);
        const double x = co * dx - s * dy, y = s * dx + co * dy;
        dx = x;
        dy = y;
    }
    c[0] = (float)((double)px + dx);
    c[1] = (float)((double)py + dy);
    c[2] = (float)((double)pz + (double)r[2]);
}

// length, width and yaw of decode_range_view (coding.py:130-144), fp64 rounded to fp32
__device__ __forceinline__ void decode_lwa(const float* r, float px, float py, int az_inv, float* lwa) {
    double yaw = atan2((double)r[6], (double)r[7]);
    if (az_inv) yaw += atan2((double)py, (double)px);
    lwa[0] = (float)exp((double)r[3]);
    lwa[1] = (float)exp((double)r[4]);
    lwa[2] = (float)yaw;
}

template <bool BEV, bool NORM>
__global__ __launch_bounds__(256) void sa_affinity_kernel(const SaTable t) {
    const int k = entry_of(t);
    const SaEntry& e = t.e[k];
    const int64_t hw = (int64_t)e.H * e.W, total = (int64_t)t.B * hw;
    const int64_t n_blocks = t.block_begin[k + 1] - t.block_begin[k];
    for (int64_t i = ((int64_t)blockIdx.x - t.block_begin[k]) * blockDim.x + threadIdx.x; i < total; i += n_blocks * blockDim.x) {
        const int64_t b = i / hw, pix = i - b * hw;
        const int64_t slot = slot_of(t, k, b, e.pan[i]);
        if (slot < 0) {
            e.map[i] = 0.f;
            continue;
        }
        const float* cart = e.cart + b * 3 * hw;
        const float px = cart[pix], py = cart[hw + pix], pz = cart[2 * hw + pix];
        float r[8], tg[8];
        const f32x4 r0 = *(const f32x4*)(e.reg + i * e.ld_reg), r1 = *(const f32x4*)(e.reg + i * e.ld_reg + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = r0[j];
            r[4 + j] = r1[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) tg[j] = e.reg_targets[(b * 8 + j) * hw + pix];
        float cp[3], cg[3];
        decode_centre(r, px, py, pz, 1, cp);  // predictions are always decoded azimuth-invariantly (assignment.py:112)
        decode_centre(tg, px, py, pz, t.az_inv, cg);
        if (BEV) {
            float lp[3], lg[3];
            decode_lwa(r, px, py, 1, lp);
            decode_lwa(tg, px, py, t.az_inv, lg);
            const float iou = bev_iou(cp, lp, cg, lg);
            e.map[i] = fminf(fmaxf(iou, 0.f), 1.f);  // (.clamp(0, 1), assignment.py:70)
        } else {
            const float dx = cp[0] - cg[0], dy = cp[1] - cg[1], dz = cp[2] - cg[2];
            const float d = sqrtf(dx * dx + dy * dy + dz * dz);
            if (NORM) {
                e.map[i] = d;
                atomicMin(&t.dmin[slot], __float_as_uint(d));
            } else {
                e.map[i] = expf(-d / (t.sigma * t.sigma));
            }
        }
    }
}

// normalize_affinities (assignment.py:158-160): dists -= dists.min(); exp(-dists / sigma^2)
__global__ __launch_bounds__(256) void sa_normalize_kernel(const SaTable t) {
    const int k = entry_of(t);
    const SaEntry& e = t.e[k];
    const int64_t hw = (int64_t)e.H * e.W, total = (int64_t)t.B * hw;
    const int64_t n_blocks = t.block_begin[k + 1] - t.block_begin[k];
    for (int64_t i = ((int64_t)blockIdx.x - t.block_begin[k]) * blockDim.x + threadIdx.x; i < total; i += n_blocks * blockDim.x) {
        const int64_t slot = slot_of(t, k, i / hw, e.pan[i]);
        if (slot < 0) continue;
        const float d = e.map[i] - __uint_as_float(t.dmin[slot]);
        e.map[i] = expf(-d / (t.sigma * t.sigma));
    }
}

// radix select, round `round` of 4: the digit is bits [24 - 8 round, 32 - 8 round) of the affinity
__global__ __launch_bounds__(256) void sa_hist_kernel(const SaTable t, int round) {
    const int k = entry_of(t);
    const SaEntry& e = t.e[k];
    const int64_t hw = (int64_t)e.H * e.W, total = (int64_t)t.B * hw;
    const int64_t n_blocks = t.block_begin[k + 1] - t.block_begin[k];
    const int shift = 24 - 8 * round;
    for (int64_t i = ((int64_t)blockIdx.x - t.block_begin[k]) * blockDim.x + threadIdx.x; i < total; i += n_blocks * blockDim.x) {
        const int64_t slot = slot_of(t, k, i / hw, e.pan[i]);
        if (slot < 0) continue;
        const uint32_t bits = __float_as_uint(e.map[i]);
        // (64-bit shifts: round 0 compares nothing)
        if (((uint64_t)(bits ^ t.prefix[slot]) >> (shift + 8)) == 0) atomicAdd(&t.hist[slot * 256 + ((bits >> shift) & 255u)], 1u);
    }
}

// one wave per slot: lane l holds the bins 4 l .. 4 l + 3.  The digit is the largest one with (values in higher bins) + (its own bin)
// >= the count still to find; an instance with fewer values than that keeps digit 0 in every round (threshold 0: everything stays).
__global__ __launch_bounds__(256) void sa_scan_kernel(const SaTable t, int round, int64_t n_slots) {
    const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= n_slots) return;
    const int lane = threadIdx.x & 63;
    u32x4* bins = (u32x4*)(t.hist + slot * 256) + lane;
    const u32x4 h = *bins;
    *bins = u32x4{0u, 0u, 0u, 0u};
    const uint32_t want = round == 0 ? (uint32_t)t.k : t.krem[slot];
    const uint32_t own = h[0] + h[1] + h[2] + h[3];
    uint32_t incl = own;  // sum over the lanes >= this one
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_down(incl, o, 64);
        if (lane + o < 64) incl += v;
    }
    const uint64_t reach = __ballot(incl >= want);  // lanes 0 .. L: the digit lies in lane L
    if (reach == 0) {
        if (lane == 0) t.krem[slot] = want;  // (prefix keeps digit 0)
        return;
    }
    if (lane != 63 - __builtin_clzll(reach)) return;
    uint32_t above = incl - own;
    int digit = 3;
    while (digit > 0 && above + h[digit] < want) above += h[digit--];
    t.prefix[slot] |= (uint32_t)(4 * lane + digit) << (24 - 8 * round);
    t.krem[slot] = want - above;
}

__global__ __launch_bounds__(256) void sa_apply_kernel(const SaTable t) {
    const int k = entry_of(t);
    const SaEntry& e = t.e[k];
    const int64_t hw = (int64_t)e.H * e.W, total = (int64_t)t.B * hw;
    const int64_t n_blocks = t.block_begin[k + 1] - t.block_begin[k];
    for (int64_t i = ((int64_t)blockIdx.x - t.block_begin[k]) * blockDim.x + threadIdx.x; i < total; i += n_blocks * blockDim.x) {
        const int64_t slot = slot_of(t, k, i / hw, e.pan[i]);
        if (slot < 0) continue;
        if (__float_as_uint(e.map[i]) < t.prefix[slot]) e.map[i] = 0.f;
    }
}

}  // namespace

extern "C" int64_t rv_soft_assign_workspace_bytes(int32_t n_entries, int32_t m, int32_t B) {
    if (n_entries < 1 || m < 0 || B < 1) return 0;
    const int64_t slots = (int64_t)n_entries * ((int64_t)m + B);
    return rv_align256(slots * (3 + 256) * (int64_t)sizeof(uint32_t));
}

extern "C" int rv_soft_assign(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params, int32_t affinity_fn,
                              int32_t normalize, int32_t k, const int32_t* box_offsets, int32_t m, void* workspace,
                              float* const* host_affinity_maps, rvStream stream) {
    RV_REQUIRE(host_entries && host_params && host_affinity_maps && box_offsets, "rv_soft_assign: null argument");
    RV_REQUIRE(n_entries >= 1 && n_entries <= RV_ML_MAX_ENTRIES, "rv_soft_assign: %d entries (1 .. %d)", n_entries, RV_ML_MAX_ENTRIES);
    RV_REQUIRE(affinity_fn == RV_AFFINITY_GAUSSIAN || affinity_fn == RV_AFFINITY_BEV, "rv_soft_assign: unknown affinity function %d", affinity_fn);
    RV_REQUIRE(!(affinity_fn == RV_AFFINITY_BEV && normalize),
               "rv_soft_assign: BEV with normalize_affinities is an UnboundLocalError in the reference (math/ops/assignment.py:71-72)");
    RV_REQUIRE(k >= 0 && m >= 0, "rv_soft_assign: k = %d (0 = infinity, else >= 1), m = %d", k, m);
    const bool select = k > 0, norm = normalize != 0;
    RV_REQUIRE(workspace || !(select || norm), "rv_soft_assign: null workspace");
    SaTable t;
    memset(&t, 0, sizeof(t));
    t.n = n_entries;
    t.B = host_entries[0].B;
    t.m = m;
    t.box_offsets = box_offsets;
    t.sigma = host_params->sigma;
    t.az_inv = host_params->azimuth_invariant;
    t.k = k;
    for (int j = 0; j < n_entries; ++j) {
        const rvLossEntry& e = host_entries[j];
        RV_REQUIRE(e.regressands && e.cart && e.panoptics && e.reg_targets && host_affinity_maps[j], "rv_soft_assign: null tensor in entry %d", j);
        RV_REQUIRE(e.B == t.B && e.B > 0 && e.H > 0 && e.W > 0, "rv_soft_assign: bad shape in entry %d (every entry has the B of box_offsets)", j);
        RV_REQUIRE(e.ld_reg >= 8 && e.ld_reg % 4 == 0, "rv_soft_assign: bad strides in entry %d (rows of regressands must be 16-byte aligned)", j);
        t.e[j] = SaEntry{e.regressands, e.cart, e.panoptics, e.reg_targets, host_affinity_maps[j], e.ld_reg, e.H, e.W};
        const int64_t blocks = ((int64_t)e.B * e.H * e.W + 255) / 256;
        t.block_begin[j + 1] = t.block_begin[j] + (int)(blocks > 2048 ? 2048 : blocks);
    }
    const int64_t slots = (int64_t)n_entries * ((int64_t)m + t.B);
    hipStream_t st = (hipStream_t)stream;
    if (select || norm) {
        RV_REQUIRE((uintptr_t)workspace % 16 == 0, "rv_soft_assign: workspace must be 16-byte aligned");
        t.hist = (uint32_t*)workspace;  // (first: sa_scan_kernel reads a slot's bins with 16-byte loads)
        t.prefix = t.hist + slots * 256;
        t.krem = t.prefix + slots;
        t.dmin = t.krem + slots;
        hipError_t err = hipMemsetAsync(workspace, 0, (size_t)slots * (3 + 256) * sizeof(uint32_t), st);
        if (err == hipSuccess && norm) err = hipMemsetAsync(t.dmin, 0xff, (size_t)slots * sizeof(uint32_t), st);
        if (err != hipSuccess) RV_FAIL("rv_soft_assign: %s", hipGetErrorString(err));
    }
    const dim3 grid(t.block_begin[n_entries]), block(256);
    if (affinity_fn == RV_AFFINITY_BEV)
        hipLaunchKernelGGL((sa_affinity_kernel<true, false>), grid, block, 0, st, t);
    else if (norm)
        hipLaunchKernelGGL((sa_affinity_kernel<false, true>), grid, block, 0, st, t);
    else
        hipLaunchKernelGGL((sa_affinity_kernel<false, false>), grid, block, 0, st, t);
    if (norm) hipLaunchKernelGGL(sa_normalize_kernel, grid, block, 0, st, t);
    if (select) {
        for (int round = 0; round < 4; ++round) {
            hipLaunchKernelGGL(sa_hist_kernel, grid, block, 0, st, t, round);
            hipLaunchKernelGGL(sa_scan_kernel, dim3((unsigned)((slots + 3) / 4)), block, 0, st, t, round, slots);
        }
        hipLaunchKernelGGL(sa_apply_kernel, grid, block, 0, st, t);
    }
    RV_CHECK_LAUNCH("soft assignment kernels");
    return 0;
}
