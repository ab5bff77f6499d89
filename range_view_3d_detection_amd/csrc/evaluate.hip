// evaluate.hip -- detection evaluation with the AV2 sensor-dataset metric definitions, on the device.
//
// The reference hands its detections to av2's CPU evaluator (nn/arch/detector.py:457-479); av2 is not part of the reference tree, so
// the semantics are DECLARED (include/rv3d.h) -- parity unpinned, as for rv_wnms.  Two entry points:
//
//   rv_eval_match      eval_match_kernel: one workgroup per (sweep, category) segment of score-sorted detections, plus one workgroup
//                      for the rows outside every segment.
//                        A  walk the segment in score order: range filter, running count (ballot scan carried over tiles), the first
//                           `cap` rows in range are the evaluated detections and go to an LDS list; every other row gets its defaults;
//                           rv_eval_match_roi (the same kernel, dt_roi given): a row in range holds its place among the `cap` whatever
//                           its flag, and only the flagged ones of them are evaluated (a second ballot scan packs the list);
//                        B  every thread owns evaluated detections (rank = k * 256 + thread) and keeps (min d2, argmin) in registers
//                           while the segment's ground truth passes through LDS in chunks of GT_CHUNK (no bound on their number);
//                        C  per chunk: LDS atomicMin of the detection's rank on its nearest ground truth; the detection that finds its
//                           own rank there is the match, every other claimant is unmatched.  Integer min: no dependence on scheduling.
//   rv_eval_summarize  eval_curve_kernel: one workgroup per (category, threshold): running true-positive count (block scan carried
//                      over tiles), right-to-left running maximum of the precision (second pass), interpolation at the sample
//                      recalls (binary search per sample), fp64 throughout; the threshold-0 workgroup of a category also sums its
//                      error columns.  eval_table_kernel: one workgroup folds the per-threshold results into the metric table.
//
// Everything below is compiled without fused multiply-add contraction (the pragma): flags are decided on fp64 squared distances formed
// as ((dx*dx + dy*dy) + dz*dz) from the fp32 inputs and have to equal NumPy's bit for bit.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

#include "segments.h"

namespace {

constexpr int THREADS = 256;
static_assert(THREADS == 64 * SEG_WAVES, "segments.h scans a workgroup of 256 threads");
constexpr int GT_CHUNK = 1024;  // ground truths staged per pass: 12 KB of centres + 4 KB of claims

struct EvalMatchArgs {
    Segments s;
    const float* dts;         // (n_dt, 10)
    const float* gts;         // (n_gt, 10)
    const uint8_t* gt_valid;  // (n_gt) or null
    const uint8_t* dt_roi;    // (n_dt) or null: rv_eval_match_roi
    int n_seg, n_thr, cap;
    double range2, tp_thr2;
    double thr2[RV_EVAL_MAX_THRESHOLDS];
    uint8_t* dt_evaluated;
    uint8_t* tp;
    float* err;
    int32_t* matched;
    uint8_t* gt_evaluated;
};

__device__ __forceinline__ double norm2(const float* row) {
    const double x = row[0], y = row[1], z = row[2];
    return (x * x + y * y) + z * z;
}

__device__ __forceinline__ double yaw_of(const float* row) { return 2.0 * atan2((double)row[9], (double)row[6]); }

__device__ __forceinline__ void write_unmatched(const EvalMatchArgs& a, int64_t row, bool evaluated) {
    a.dt_evaluated[row] = evaluated ? 1 : 0;
    for (int t = 0; t < a.n_thr; ++t) a.tp[row * a.n_thr + t] = 0;
    for (int k = 0; k < 3; ++k) a.err[row * 3 + k] = __builtin_nanf("");
    a.matched[row] = -1;
}

// rows of [lo, hi) in sorted order that belong to no segment: not evaluated
__device__ void write_outside(const EvalMatchArgs& a, int64_t dlo, int64_t dhi, int64_t glo, int64_t ghi) {
    for (int64_t i = dlo + threadIdx.x; i < dhi; i += THREADS) {
        const int64_t row = row_at(a.s.dt_order, i, a.s.n_dt);
        if (row >= 0) write_unmatched(a, row, false);
    }
    for (int64_t i = glo + threadIdx.x; i < ghi; i += THREADS) {
        const int64_t row = row_at(a.s.gt_order, i, a.s.n_gt);
        if (row >= 0) a.gt_evaluated[row] = 0;
    }
}

__global__ __launch_bounds__(THREADS) void eval_match_kernel(const EvalMatchArgs a) {
    __shared__ int64_t ev_row[RV_EVAL_MAX_DTS];  // evaluated detections of the segment, by rank
    __shared__ double ev_d2[RV_EVAL_MAX_DTS];    // squared distance to the nearest evaluated ground truth
    __shared__ int ev_best[RV_EVAL_MAX_DTS];     // its index in the segment, or -1
    __shared__ float gt_xyz[GT_CHUNK * 3];
    __shared__ int claim[GT_CHUNK];
    __shared__ int wave_count[SEG_WAVES];
    const int tid = threadIdx.x;
    const int seg = blockIdx.x;
    if (seg == a.n_seg) {  // the rows before the first segment and behind the last one
        const Bounds first = bounds_of(a.s, 0), last = bounds_of(a.s, a.n_seg - 1);
        write_outside(a, 0, first.d0, 0, first.g0);
        write_outside(a, last.d0 + last.nd, a.s.n_dt, last.g0 + last.ng, a.s.n_gt);
        return;
    }
    const Bounds b = bounds_of(a.s, seg);
    const int64_t d0 = b.d0, d1 = b.d0 + b.nd, g0 = b.g0, g1 = b.g0 + b.ng;

    // A: the first `cap` rows in range, in score order
    int n_eval = 0, n_kept = 0;  // rows in range so far; with dt_roi: the evaluated ones among them
    for (int64_t base = d0; base < d1; base += THREADS) {
        const int64_t i = base + tid;
        const int64_t row = i < d1 ? row_at(a.s.dt_order, i, a.s.n_dt) : -1;
        const bool in_range = row >= 0 && norm2(a.dts + row * 10) <= a.range2;
        int total;
        const int rank = tile_rank(in_range, n_eval, wave_count, &total);
        bool evaluated = in_range && rank < a.cap;
        int slot = rank;
        if (a.dt_roi) {  // (the same for the whole grid) cap first, then the ROI flag: the evaluated rows are packed by a second scan
            evaluated = evaluated && a.dt_roi[row] != 0;
            int kept;
            slot = tile_rank(evaluated, n_kept, wave_count, &kept);
            n_kept += kept;
        }
        if (evaluated) ev_row[slot] = row;
        else if (row >= 0) write_unmatched(a, row, false);
        n_eval += total;
    }
    if (n_eval > a.cap) n_eval = a.cap;
    if (a.dt_roi) n_eval = n_kept;
    __syncthreads();  // (B reads ranks that other threads wrote)

    // B: nearest evaluated ground truth of every evaluated detection (ties: the lowest index, `<` below)
    const int n_pass = n_eval > 0 ? (n_eval + THREADS - 1) / THREADS : 1;  // (one pass with no detections still flags the ground truth)
    for (int pass = 0; pass < n_pass; ++pass) {
        const int rank = pass * THREADS + tid;
        double x = 0., y = 0., z = 0., best = INFINITY;
        int best_g = -1;
        if (rank < n_eval) {
            const float* d = a.dts + ev_row[rank] * 10;
            x = d[0], y = d[1], z = d[2];
        }
        for (int64_t c0 = g0; c0 < g1; c0 += GT_CHUNK) {
            const int n_c = (int)(g1 - c0 < GT_CHUNK ? g1 - c0 : GT_CHUNK);
            __syncthreads();
            for (int j = tid; j < n_c; j += THREADS) {
                const int64_t row = row_at(a.s.gt_order, c0 + j, a.s.n_gt);
                bool evaluated = false;
                if (row >= 0) {
                    const float* g = a.gts + row * 10;
                    evaluated = (!a.gt_valid || a.gt_valid[row]) && norm2(g) <= a.range2;
                    if (pass == 0) a.gt_evaluated[row] = evaluated ? 1 : 0;
                    gt_xyz[3 * j + 1] = g[1];
                    gt_xyz[3 * j + 2] = g[2];
                    gt_xyz[3 * j] = evaluated ? g[0] : __builtin_nanf("");  // a NaN distance never compares below `best`
                } else {
                    gt_xyz[3 * j] = __builtin_nanf("");
                }
            }
            __syncthreads();
            if (rank < n_eval) {
                for (int j = 0; j < n_c; ++j) {  // (every lane reads the same LDS words: broadcast)
                    const double dx = x - (double)gt_xyz[3 * j], dy = y - (double)gt_xyz[3 * j + 1], dz = z - (double)gt_xyz[3 * j + 2];
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < best) best = d2, best_g = (int)(c0 - g0) + j;
                }
            }
        }
        if (rank < n_eval) ev_d2[rank] = best, ev_best[rank] = best_g;
    }
    __syncthreads();

    // C: a ground truth goes to the first detection in score order that picked it; the others stay unmatched
    for (int64_t c0 = g0; c0 < g1; c0 += GT_CHUNK) {
        const int lo = (int)(c0 - g0);
        for (int j = tid; j < GT_CHUNK; j += THREADS) claim[j] = 0x7fffffff;
        __syncthreads();
        for (int rank = tid; rank < n_eval; rank += THREADS) {
            const int g = ev_best[rank] - lo;
            if (ev_best[rank] >= 0 && g >= 0 && g < GT_CHUNK) atomicMin(&claim[g], rank);
        }
        __syncthreads();
        for (int rank = tid; rank < n_eval; rank += THREADS) {
            const int g = ev_best[rank] - lo;
            if (ev_best[rank] < 0 || g < 0 || g >= GT_CHUNK) continue;
            const int64_t row = ev_row[rank];
            if (claim[g] != rank) {
                write_unmatched(a, row, true);
                continue;
            }
            const int64_t gt_row = a.s.gt_order[c0 + g];  // (in range: this entry was staged as evaluated)
            const double d2 = ev_d2[rank];
            a.dt_evaluated[row] = 1;
            a.matched[row] = (int32_t)gt_row;
            for (int t = 0; t < a.n_thr; ++t) a.tp[row * a.n_thr + t] = d2 <= a.thr2[t] ? 1 : 0;
            if (d2 <= a.tp_thr2) {
                const float* d = a.dts + row * 10;
                const float* g_ = a.gts + gt_row * 10;
                // ASE: 1 - IoU of the boxes aligned in centre and heading (math/ops/iou.py:50-55: prod(min) / prod(max))
                double inter = 1., uni = 1.;
                for (int k = 3; k < 6; ++k) {
                    const double p = d[k], q = g_[k];
                    inter *= p < q ? p : q;
                    uni *= p < q ? q : p;
                }
                // AOE: |yaw difference| wrapped to [0, pi]
                double dyaw = fabs(yaw_of(d) - yaw_of(g_));
                dyaw = fmod(dyaw, 2.0 * M_PI);
                if (dyaw > M_PI) dyaw = 2.0 * M_PI - dyaw;
                a.err[row * 3] = (float)sqrt(d2);
                a.err[row * 3 + 1] = (float)(1.0 - inter / uni);
                a.err[row * 3 + 2] = (float)dyaw;
            } else {
                for (int k = 0; k < 3; ++k) a.err[row * 3 + k] = __builtin_nanf("");
            }
        }
        __syncthreads();
    }
    for (int rank = tid; rank < n_eval; rank += THREADS)  // no evaluated ground truth in the segment
        if (ev_best[rank] < 0) write_unmatched(a, ev_row[rank], true);
}

// ---------------------------------------------------------------------------------------
// summary
// ---------------------------------------------------------------------------------------
struct EvalSumArgs {
    const uint8_t* flags;    // (n_rows, n_thr), rows of a category contiguous and score-sorted
    const float* err;        // (n_rows, 3)
    const int64_t* cat_off;  // (n_cat + 1)
    const int64_t* n_gt;     // (n_cat)
    int64_t n_rows;
    int n_cat, n_thr, n_samples;
    double tp_thr, default_ase, default_aoe;
    int32_t* cum;      // workspace (n_thr, n_rows): running true-positive count
    double* pmax;      // workspace (n_thr, n_rows): precision, non-increasing from the right
    double* err_sums;  // workspace (n_cat, 4): sums of the three error columns over the true positives, their number
    double* table;     // (n_cat + 1, 5)
    double* ap_t;      // (n_cat, n_thr)
};

// inclusive scan over the 256 threads in thread order; `scratch` holds one value per wave
template <class T, class Op>
__device__ __forceinline__ T block_scan(T v, Op op, T* scratch, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v = op(u, v);
    }
    __syncthreads();  // (scratch may still be read from the tile before)
    if (lane == 63) scratch[wave] = v;
    __syncthreads();
    T all = scratch[0];
    for (int w = 1; w < THREADS / 64; ++w) {
        if (w == wave) v = op(all, v);
        all = op(all, scratch[w]);
    }
    *total = all;
    return v;
}

__global__ __launch_bounds__(THREADS) void eval_curve_kernel(const EvalSumArgs a) {
    __shared__ int scratch_i[THREADS / 64];
    __shared__ double scratch_d[THREADS / 64];
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int64_t r0 = clamp64(a.cat_off[c], 0, a.n_rows), r1 = clamp64(a.cat_off[c + 1], r0, a.n_rows);
    const int64_t n = r1 - r0, n_gt = a.n_gt[c];
    int32_t* cum = a.cum + (int64_t)t * a.n_rows + r0;
    double* pmax = a.pmax + (int64_t)t * a.n_rows + r0;

    if (t == 0) {  // error sums over the true positives at tp_threshold_m (the rows whose errors are not NaN)
        double s[3] = {0., 0., 0.}, cnt = 0.;
        for (int64_t i = tid; i < n; i += THREADS) {
            const float* e = a.err + (r0 + i) * 3;
            if (e[0] == e[0]) s[0] += (double)e[0], s[1] += (double)e[1], s[2] += (double)e[2], cnt += 1.;
        }
        for (int k = 0; k < 3; ++k) s[k] = block_sum(s[k], scratch_d);
        cnt = block_sum(cnt, scratch_d);
        if (tid == 0) {
            for (int k = 0; k < 3; ++k) a.err_sums[c * 4 + k] = s[k];
            a.err_sums[c * 4 + 3] = cnt;
        }
    }
    if (n == 0 || n_gt <= 0) {
        if (tid == 0) a.ap_t[c * a.n_thr + t] = 0.;
        return;
    }
    // 1: tp = cumsum(flag)
    int carry = 0;
    for (int64_t base = 0; base < n; base += THREADS) {
        const int64_t i = base + tid;
        int total;
        const int v = block_scan<int>(i < n ? (a.flags[(r0 + i) * a.n_thr + t] != 0) : 0, [](int p, int q) { return p + q; }, scratch_i, &total);
        if (i < n) cum[i] = carry + v;
        carry += total;
    }
    __syncthreads();  // (pass 2 reads counts that other threads of the workgroup wrote)
    // 2: precision = tp / (tp + fp), made non-increasing from the right
    double right = 0.;  // (precisions are >= 0)
    for (int64_t top = n; top > 0; top -= THREADS) {
        const int64_t i = top - 1 - tid;  // thread order = right to left
        double total;
        const double p = i >= 0 ? (double)cum[i] / (double)(i + 1) : 0.;
        const double v = block_scan<double>(p, [](double u, double w) { return u > w ? u : w; }, scratch_d, &total);
        if (i >= 0) pmax[i] = v > right ? v : right;
        right = total > right ? total : right;
    }
    __syncthreads();
    // 3: np.interp(linspace(0, 1, n_samples), recall, precision, left = precision[0], right = 0), then the mean
    const double step = a.n_samples > 1 ? 1.0 / (double)(a.n_samples - 1) : 0.;
    const double xp_last = (double)cum[n - 1] / (double)n_gt, xp_first = (double)cum[0] / (double)n_gt;
    double acc = 0.;
    for (int s = tid; s < a.n_samples; s += THREADS) {
        const double x = s == a.n_samples - 1 && s > 0 ? 1.0 : (double)s * step;
        double y;
        if (x > xp_last) y = 0.;
        else if (x < xp_first) y = pmax[0];
        else {
            int64_t lo = 0, hi = n;  // the last j with recall[j] <= x
            while (hi - lo > 1) {
                const int64_t mid = lo + (hi - lo) / 2;
                if ((double)cum[mid] / (double)n_gt <= x) lo = mid;
                else hi = mid;
            }
            const double xl = (double)cum[lo] / (double)n_gt;
            if (lo == n - 1 || xl == x) y = pmax[lo];
            else {
                const double slope = (pmax[lo + 1] - pmax[lo]) / ((double)cum[lo + 1] / (double)n_gt - xl);
                y = slope * (x - xl) + pmax[lo];
            }
        }
        acc += y;
    }
    acc = block_sum(acc, scratch_d);
    if (tid == 0) a.ap_t[c * a.n_thr + t] = acc / (double)a.n_samples;
}

__global__ __launch_bounds__(THREADS) void eval_table_kernel(const EvalSumArgs a) {
    __shared__ double scratch_d[THREADS / 64];
    double col[5] = {0., 0., 0., 0., 0.};
    for (int c = threadIdx.x; c < a.n_cat; c += THREADS) {
        double ap = 0.;
        for (int t = 0; t < a.n_thr; ++t) ap += a.ap_t[c * a.n_thr + t];
        ap /= (double)a.n_thr;
        const double* s = a.err_sums + c * 4;
        double m[5] = {ap, a.tp_thr, a.default_ase, a.default_aoe, 0.};
        if (s[3] > 0.)
            for (int k = 0; k < 3; ++k) m[1 + k] = s[k] / s[3];
        const double ate = m[1] / a.tp_thr, aoe = m[3] / M_PI;
        m[4] = ap * (((1. - (ate < 1. ? ate : 1.)) + (1. - (m[2] < 1. ? m[2] : 1.)) + (1. - (aoe < 1. ? aoe : 1.))) / 3.);
        for (int k = 0; k < 5; ++k) a.table[c * 5 + k] = m[k], col[k] += m[k];
    }
    for (int k = 0; k < 5; ++k) {
        const double s = block_sum(col[k], scratch_d);
        if (threadIdx.x == 0) a.table[a.n_cat * 5 + k] = s / (double)a.n_cat;
    }
}

}  // namespace

namespace {

int eval_match(const float* dts, const int64_t* dt_order, const int64_t* dt_offsets, int64_t n_dt, const float* gts, const uint8_t* gt_valid,
               const int64_t* gt_order, const int64_t* gt_offsets, int64_t n_gt, int32_t n_segments, const double* host_thresholds_m,
               int32_t n_thresholds, double tp_threshold_m, double max_range_m, int32_t max_num_dts, const uint8_t* dt_roi, uint8_t* dt_evaluated,
               uint8_t* tp, float* err, int32_t* matched_gt, uint8_t* gt_evaluated, rvStream stream) {
    RV_REQUIRE(n_dt >= 0 && n_gt >= 0 && n_gt <= 0x7fffffff, "rv_eval_match: n_dt = %lld, n_gt = %lld", (long long)n_dt, (long long)n_gt);
    RV_REQUIRE(n_segments >= 1, "rv_eval_match: %d segments", n_segments);
    RV_REQUIRE(host_thresholds_m && n_thresholds >= 1 && n_thresholds <= RV_EVAL_MAX_THRESHOLDS, "rv_eval_match: %d thresholds (1 .. %d)",
               n_thresholds, RV_EVAL_MAX_THRESHOLDS);
    RV_REQUIRE(max_num_dts >= 1 && max_num_dts <= RV_EVAL_MAX_DTS, "rv_eval_match: max_num_dts = %d (1 .. %d)", max_num_dts, RV_EVAL_MAX_DTS);
    RV_REQUIRE(tp_threshold_m > 0. && max_range_m >= 0., "rv_eval_match: tp_threshold_m = %g, max_range_m = %g", tp_threshold_m, max_range_m);
    RV_REQUIRE(dt_offsets && gt_offsets, "rv_eval_match: null segment offsets");
    RV_REQUIRE(n_dt == 0 || (dts && dt_order && dt_evaluated && tp && err && matched_gt), "rv_eval_match: null detection buffer");
    RV_REQUIRE(n_gt == 0 || (gts && gt_order && gt_evaluated), "rv_eval_match: null ground-truth buffer");
    EvalMatchArgs a;
    memset(&a, 0, sizeof(a));
    a.s = Segments{dt_order, dt_offsets, gt_order, gt_offsets, n_dt, n_gt};
    a.dts = dts, a.gts = gts, a.gt_valid = gt_valid, a.dt_roi = n_dt > 0 ? dt_roi : nullptr;
    a.n_seg = n_segments, a.n_thr = n_thresholds, a.cap = max_num_dts;
    a.range2 = max_range_m * max_range_m;
    a.tp_thr2 = tp_threshold_m * tp_threshold_m;
    for (int t = 0; t < n_thresholds; ++t) {
        RV_REQUIRE(host_thresholds_m[t] >= 0., "rv_eval_match: threshold %d is %g", t, host_thresholds_m[t]);
        a.thr2[t] = host_thresholds_m[t] * host_thresholds_m[t];
    }
    a.dt_evaluated = dt_evaluated, a.tp = tp, a.err = err, a.matched = matched_gt, a.gt_evaluated = gt_evaluated;
    hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)n_segments + 1), dim3(THREADS), 0, (hipStream_t)stream, a);
    RV_CHECK_LAUNCH("eval_match_kernel");
    return 0;
}

}  // namespace

extern "C" int rv_eval_match(const float* dts, const int64_t* dt_order, const int64_t* dt_offsets, int64_t n_dt, const float* gts,
                             const uint8_t* gt_valid, const int64_t* gt_order, const int64_t* gt_offsets, int64_t n_gt, int32_t n_segments,
                             const double* host_thresholds_m, int32_t n_thresholds, double tp_threshold_m, double max_range_m,
                             int32_t max_num_dts, uint8_t* dt_evaluated, uint8_t* tp, float* err, int32_t* matched_gt, uint8_t* gt_evaluated,
                             rvStream stream) {
    return eval_match(dts, dt_order, dt_offsets, n_dt, gts, gt_valid, gt_order, gt_offsets, n_gt, n_segments, host_thresholds_m, n_thresholds,
                      tp_threshold_m, max_range_m, max_num_dts, nullptr, dt_evaluated, tp, err, matched_gt, gt_evaluated, stream);
}

// the same kernel with the detections' ROI flags (include/rv3d.h: cap first, then the flag); dt_roi == NULL is rv_eval_match
extern "C" int rv_eval_match_roi(const float* dts, const int64_t* dt_order, const int64_t* dt_offsets, int64_t n_dt, const float* gts,
                                 const uint8_t* gt_valid, const int64_t* gt_order, const int64_t* gt_offsets, int64_t n_gt, int32_t n_segments,
                                 const double* host_thresholds_m, int32_t n_thresholds, double tp_threshold_m, double max_range_m,
                                 int32_t max_num_dts, const uint8_t* dt_roi, uint8_t* dt_evaluated, uint8_t* tp, float* err, int32_t* matched_gt,
                                 uint8_t* gt_evaluated, rvStream stream) {
    return eval_match(dts, dt_order, dt_offsets, n_dt, gts, gt_valid, gt_order, gt_offsets, n_gt, n_segments, host_thresholds_m, n_thresholds,
                      tp_threshold_m, max_range_m, max_num_dts, dt_roi, dt_evaluated, tp, err, matched_gt, gt_evaluated, stream);
}

extern "C" int64_t rv_eval_summarize_workspace_bytes(int64_t n_rows, int32_t n_categories, int32_t n_thresholds) {
    if (n_rows < 0 || n_categories < 1 || n_thresholds < 1) return 0;
    return rv_align256(n_rows * n_thresholds * (int64_t)sizeof(double)) + rv_align256(n_rows * n_thresholds * (int64_t)sizeof(int32_t)) +
           rv_align256((int64_t)n_categories * 4 * (int64_t)sizeof(double));
}

extern "C" int rv_eval_summarize(const uint8_t* flags, const float* err, const int64_t* cat_offsets, const int64_t* n_gt, int64_t n_rows,
                                 int32_t n_categories, int32_t n_thresholds, double tp_threshold_m, int32_t num_recall_samples,
                                 double default_ase, double default_aoe, void* workspace, double* table, double* ap_per_threshold,
                                 rvStream stream) {
    RV_REQUIRE(n_rows >= 0 && n_rows <= 0x7fffffff, "rv_eval_summarize: %lld rows (the running counts are 32-bit)", (long long)n_rows);
    RV_REQUIRE(n_categories >= 1 && n_categories <= 65535, "rv_eval_summarize: %d categories", n_categories);
    RV_REQUIRE(n_thresholds >= 1 && n_thresholds <= RV_EVAL_MAX_THRESHOLDS, "rv_eval_summarize: %d thresholds (1 .. %d)", n_thresholds,
               RV_EVAL_MAX_THRESHOLDS);
    RV_REQUIRE(num_recall_samples >= 1 && tp_threshold_m > 0., "rv_eval_summarize: num_recall_samples = %d, tp_threshold_m = %g",
               num_recall_samples, tp_threshold_m);
    RV_REQUIRE(cat_offsets && n_gt && workspace && table && ap_per_threshold, "rv_eval_summarize: null argument");
    RV_REQUIRE(n_rows == 0 || (flags && err), "rv_eval_summarize: null row buffer");
    RV_REQUIRE((uintptr_t)workspace % 8 == 0, "rv_eval_summarize: workspace must be 8-byte aligned");
    EvalSumArgs a;
    memset(&a, 0, sizeof(a));
    a.flags = flags, a.err = err, a.cat_off = cat_offsets, a.n_gt = n_gt, a.n_rows = n_rows;
    a.n_cat = n_categories, a.n_thr = n_thresholds, a.n_samples = num_recall_samples;
    a.tp_thr = tp_threshold_m, a.default_ase = default_ase, a.default_aoe = default_aoe;
    char* ws = (char*)workspace;
    a.pmax = (double*)ws;
    ws += rv_align256(n_rows * n_thresholds * (int64_t)sizeof(double));
    a.cum = (int32_t*)ws;
    ws += rv_align256(n_rows * n_thresholds * (int64_t)sizeof(int32_t));
    a.err_sums = (double*)ws;
    a.table = table, a.ap_t = ap_per_threshold;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_curve_kernel, dim3((unsigned)n_categories, (unsigned)n_thresholds), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL(eval_table_kernel, dim3(1), dim3(THREADS), 0, st, a);
    RV_CHECK_LAUNCH("evaluation summary kernels");
    return 0;
}
