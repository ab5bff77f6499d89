// segments.h -- the device side of the evaluators' row contract (evaluation/rows.py): the host hands over an order of the rows and
// (n_seg + 1) offsets into it, and a workgroup of 256 threads walks order[off[seg] .. off[seg + 1]).  Neither array is trusted: offsets
// are clamped to the row count and to each other, and an entry of the order that names no row is skipped.  With it, the two
// workgroup-wide primitives those walks use.  Include after common.h and after the file's `#pragma clang fp contract(off)`.
#pragma once

namespace {

constexpr int SEG_WAVES = 4;  // 256 threads

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// row of `order[i]`, or -1 when it does not name a row (nothing is read or written through such an entry)
__device__ __forceinline__ int64_t row_at(const int64_t* order, int64_t i, int64_t n) {
    const int64_t r = order[i];
    return r >= 0 && r < n ? r : -1;
}

struct Segments {
    const int64_t* dt_order;  // (n_dt): position in (segment, score) order -> row
    const int64_t* dt_off;    // (n_seg + 1)
    const int64_t* gt_order;  // (n_gt)
    const int64_t* gt_off;    // (n_seg + 1)
    int64_t n_dt, n_gt;
};

struct Bounds {
    int64_t d0, g0;  // first position of the segment in either order
    int64_t nd, ng;  // its rows
};

// segment `seg` of 0 .. n_seg - 1
__device__ __forceinline__ Bounds bounds_of(const Segments& s, int64_t seg) {
    Bounds b;
    b.d0 = clamp64(s.dt_off[seg], 0, s.n_dt);
    b.nd = clamp64(s.dt_off[seg + 1], b.d0, s.n_dt) - b.d0;
    b.g0 = clamp64(s.gt_off[seg], 0, s.n_gt);
    b.ng = clamp64(s.gt_off[seg + 1], b.g0, s.n_gt) - b.g0;
    return b;
}

// position of every set flag among the set flags of the workgroup's tile, in thread order; `base` carries over tiles
__device__ __forceinline__ int tile_rank(bool flag, int base, int* wave_count, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long votes = __ballot(flag);
    __syncthreads();  // (wave_count may still be read from the tile before)
    if (lane == 0) wave_count[wave] = __popcll(votes);
    __syncthreads();
    int rank = base + __popcll(votes & ((1ull << lane) - 1ull));
    int all = 0;
    for (int w = 0; w < SEG_WAVES; ++w) {
        if (w < wave) rank += wave_count[w];
        all += wave_count[w];
    }
    *total = all;
    return rank;
}

// sum over the 256 threads in a fixed order (wave butterfly, then the waves in order): the same bits on every run
__device__ __forceinline__ double block_sum(double v, double* scratch) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = scratch[0];
    for (int w = 1; w < SEG_WAVES; ++w) s += scratch[w];
    return s;
}

}  // namespace
