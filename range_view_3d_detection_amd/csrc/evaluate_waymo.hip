// evaluate_waymo.hip -- the Waymo Open Dataset detection metric on the device: pairwise rotated BEV / 3-D IoU, maximum-weight matching
// at all 101 score cutoffs in one pass, TP / FP / FN / heading counts per breakdown row and level, AP and APH.
//
// The reference hands its detections to waymo_open_dataset's evaluator (evaluation/evaluate.py); that library is not part of the
// reference tree, so the semantics are DECLARED (include/rv3d.h) -- parity unpinned, as for rv_eval_match.  Three entries:
//
//   rv_waymo_iou        waymo_offsets_kernel (one workgroup: the pair offsets of the segments, a scan) + waymo_iou_kernel: one thread
//                       per (detection, ground truth) pair of equal (sweep, type), grid-stride; circumscribed circles first, then the
//                       clipping of nms_geom.h; writes (BEV, 3-D) as one 8-byte store.
//   rv_waymo_match      waymo_match_kernel: one workgroup per (sweep, type, box type, range shard) problem.
//                         1  rows of the shard, their cutoff index, the gated pairs (weight > 0); LDS flags by integer atomicOr;
//                         2  ordered compaction (ballot scan) of the rows and ground truth that have a gated pair: the others never
//                            enter an augmenting path (rv3d.h says why) and are counted directly;
//                         3  rows inserted in score order, one shortest-augmenting-path search each: potentials, owners and
//                            back-pointers in LDS, every thread owns the columns tid, tid + 256, ... (their running minima and
//                            potentials stay in registers), (minimum, lowest column) through wave shuffles + four LDS slots, thread 0
//                            walks the path; after the last row of a cutoff group the workgroup counts;
//                         4  the 101 x 2 x 4 counts of the problem are added to the global tables with 64-bit integer atomics.
//   rv_waymo_summarize  waymo_summary_kernel: one workgroup per (box type, result row), one thread per cutoff, thread 0 integrates.
//
// Every loop is bounded by the segment sizes; a bound that is hit, a segment beyond RV_WAYMO_MAX_DTS / RV_WAYMO_MAX_GTS or offsets that
// do not fit the workspace set an error word and the workgroup leaves.  No workgroup waits for another.  Compiled without fused
// multiply-add contraction (the pragma): the BEV column is rv_rotated_iou's bit for bit, range shards are decided on fp64 squares.
#include "common.h"

#include <math.h>

#pragma clang fp contract(off)

#include "nms_geom.h"
#include "segments.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int COLS = RV_WAYMO_MAX_GTS / THREADS;  // columns a thread owns
constexpr int N_CUT = RV_WAYMO_NUM_CUTOFFS;
constexpr int N_ROWS = RV_WAYMO_NUM_BREAKDOWN_ROWS;
constexpr int BIG = 0x3fffffff;
constexpr int START = -2, NONE = -1;  // back-pointer of a column reached from the inserted row; "unmatched"
enum { ERR_DTS = 0, ERR_GTS = 1, ERR_WORKSPACE = 2, ERR_BOUND = 3 };

static_assert(RV_WAYMO_MAX_GTS % THREADS == 0 && RV_WAYMO_MAX_DTS % THREADS == 0, "limits are multiples of the workgroup size");
static_assert(WAVES == SEG_WAVES, "segments.h scans a workgroup of 256 threads");

// pairs of a segment in the table: none for a segment beyond a limit (rv_waymo_match reports it)
__device__ __forceinline__ int64_t pairs_of(const Bounds& b) {
    return b.nd <= RV_WAYMO_MAX_DTS && b.ng <= RV_WAYMO_MAX_GTS ? b.nd * b.ng : 0;
}

// ---------------------------------------------------------------------------------------
// pairwise IoU
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void waymo_offsets_kernel(const Segments s, int n_seg, int64_t* pair_off) {
    __shared__ int64_t part[THREADS];
    const int tid = threadIdx.x;
    const int chunk = (n_seg + THREADS - 1) / THREADS;
    const int s0 = tid * chunk < n_seg ? tid * chunk : n_seg, s1 = s0 + chunk < n_seg ? s0 + chunk : n_seg;
    int64_t sum = 0;
    for (int k = s0; k < s1; ++k) sum += pairs_of(bounds_of(s, k));
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int64_t acc = 0;
        for (int t = 0; t < THREADS; ++t) {
            const int64_t v = part[t];
            part[t] = acc;
            acc += v;
        }
        pair_off[n_seg] = acc;
    }
    __syncthreads();
    int64_t acc = part[tid];
    for (int k = s0; k < s1; ++k) {
        pair_off[k] = acc;
        acc += pairs_of(bounds_of(s, k));
    }
}

__global__ __launch_bounds__(THREADS) void waymo_iou_kernel(const Segments s, const float* dts, const float* gts, int n_seg,
                                                            const int64_t* pair_off, int64_t capacity, float2* iou) {
    int64_t total = pair_off[n_seg];
    if (total > capacity) total = capacity;  // (offsets that do not fit: rv_waymo_match reports them)
    for (int64_t p = blockIdx.x * (int64_t)THREADS + threadIdx.x; p < total; p += (int64_t)gridDim.x * THREADS) {
        int lo = 0, hi = n_seg;  // the segment with pair_off[seg] <= p < pair_off[seg + 1]
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (pair_off[mid] <= p) lo = mid;
            else hi = mid;
        }
        const Bounds b = bounds_of(s, lo);
        const int64_t local = p - pair_off[lo];
        float2 v = make_float2(0.0f, 0.0f);
        if (b.ng > 0 && local >= 0 && local < pairs_of(b)) {
            const int64_t i = local / b.ng, j = local - i * b.ng;
            const int64_t d = row_at(s.dt_order, b.d0 + i, s.n_dt), g = row_at(s.gt_order, b.g0 + j, s.n_gt);
            if (d >= 0 && g >= 0) v = waymo_iou_pair(dts + d * 7, gts + g * 7);
        }
        iou[p] = v;
    }
}

// ---------------------------------------------------------------------------------------
// matching and counts
// ---------------------------------------------------------------------------------------
struct WaymoMatchArgs {
    Segments s;
    const float* dts;     // (n_dt, 7)
    const float* scores;  // (n_dt)
    const float* gts;     // (n_gt, 7)
    const uint8_t* gt_level;     // (n_gt): 0 = not evaluated
    const uint8_t* sweep_valid;  // (n_sweeps) or null
    const int64_t* pair_off;
    const float* iou;  // (pairs, 2)
    int64_t capacity;
    float thr[5];
    unsigned long long* tables;  // (2, N_ROWS, 2, N_CUT, 4)
    int* errors;                 // (4)
};

__device__ __forceinline__ int weight_of(const float* iou, int64_t pair, int box, float thr) {
    const float v = iou[pair * 2 + box];
    if (!(v >= thr)) return 0;
    const int w = (int)floorf(1000.0f * v);
    return w > 1000 ? 1000 : (w < 0 ? 0 : w);
}

// 1 [0, 30), 2 [30, 50), 3 [50, inf) by the row's own centre; 0 = in no range shard (a NaN centre)
__device__ __forceinline__ int range_shard(const float* box) {
    const double x = box[0], y = box[1], z = box[2];
    const double r2 = (x * x + y * y) + z * z;
    return r2 < 900.0 ? 1 : (r2 < 2500.0 ? 2 : (r2 >= 2500.0 ? 3 : 0));
}

// heading accuracy of a pair as a multiple of 2^-40: 1 - |yaw difference wrapped to [0, pi]| / pi
__device__ __forceinline__ long long heading_quanta(float yaw_d, float yaw_g) {
    double d = fabs((double)yaw_d - (double)yaw_g);
    d = fmod(d, 2.0 * M_PI);
    if (d > M_PI) d = 2.0 * M_PI - d;
    const double acc = 1.0 - d / M_PI;
    if (!(acc >= 0.0)) return 0;  // (NaN yaw)
    return (long long)rint(acc * 1099511627776.0);
}

__global__ __launch_bounds__(THREADS) void waymo_match_kernel(const WaymoMatchArgs a) {
    __shared__ int u[RV_WAYMO_MAX_DTS];        // potential of a compact row
    __shared__ int col_of[RV_WAYMO_MAX_DTS];   // compact row -> compact column or NONE
    __shared__ int row_pos[RV_WAYMO_MAX_DTS];  // compact row -> position in the segment
    __shared__ int dt_flag[RV_WAYMO_MAX_DTS];  // by position: bit 0 in the problem, bit 1 has a gated pair; bits 8.. cutoff index + 1
    __shared__ int gt_flag[RV_WAYMO_MAX_GTS];  // by position: bit 0, bit 1 as above; bits 8.. level
    __shared__ int col_pos[RV_WAYMO_MAX_GTS];  // compact column -> position in the segment
    __shared__ int owner[RV_WAYMO_MAX_GTS];    // compact column -> compact row or NONE
    __shared__ int way[RV_WAYMO_MAX_GTS];      // back-pointer of the current search: the column before, or START
    __shared__ signed char row_k[RV_WAYMO_MAX_DTS];  // cutoff index of a compact row
    __shared__ unsigned char col_lvl[RV_WAYMO_MAX_GTS];
    __shared__ float cut[N_CUT];
    __shared__ int hist[N_CUT];            // rows of the problem by cutoff index, then (suffix sum) rows inserted at a cutoff
    __shared__ int cnt[N_CUT][3];          // matched, TP level 1, TP level 2
    __shared__ long long head[N_CUT][2];   // heading sums of the TPs at level 1, 2
    __shared__ int acc_i[5];               // matched, TP 1, TP 2 of a count; ground truth of level <= 1, <= 2
    __shared__ unsigned long long acc_h[2];
    __shared__ int red_val[WAVES], red_col[WAVES], wave_count[WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int shard = blockIdx.x & 3, box = (blockIdx.x >> 2) & 1;
    const int64_t seg = blockIdx.x >> 3;
    const int type = (int)(seg & 3) + 1;
    const int64_t sweep = seg >> 2;
    if (a.sweep_valid && !a.sweep_valid[sweep]) return;  // no ground truth left in the sweep: not a frame
    const Bounds b = bounds_of(a.s, seg);
    if (b.nd > RV_WAYMO_MAX_DTS || b.ng > RV_WAYMO_MAX_GTS) {  // counted once per segment
        if (tid == 0 && box == 0 && shard == 0) atomicAdd(&a.errors[b.nd > RV_WAYMO_MAX_DTS ? ERR_DTS : ERR_GTS], 1);
        return;
    }
    const int nd = (int)b.nd, ng = (int)b.ng;
    const int64_t base = a.pair_off[seg];
    if (base < 0 || base + (int64_t)nd * ng > a.capacity || a.pair_off[seg + 1] - base != (int64_t)nd * ng) {
        if (tid == 0 && box == 0 && shard == 0) atomicAdd(&a.errors[ERR_WORKSPACE], 1);
        return;
    }
    const float thr = a.thr[type];
    const int brow = shard == 0 ? type - 1 : 4 + (type - 1) * 3 + (shard - 1);

    // 1: rows and ground truth of the problem
    for (int k = tid; k < N_CUT; k += THREADS) cut[k] = k == N_CUT - 1 ? 1.0f : (float)((double)k * 0.01), hist[k] = 0;
    if (tid < 5) acc_i[tid] = 0;
    __syncthreads();
    {
        int n1 = 0, n2 = 0;
        for (int j = tid; j < ng; j += THREADS) {
            const int64_t row = row_at(a.s.gt_order, b.g0 + j, a.s.n_gt);
            int f = 0;
            if (row >= 0 && a.gt_level[row] != 0 && (shard == 0 || range_shard(a.gts + row * 7) == shard)) {
                const int lvl = a.gt_level[row];
                f = 1 | (lvl << 8);
                n1 += lvl <= 1, n2 += lvl <= 2;
            }
            gt_flag[j] = f;
        }
        if (n1) atomicAdd(&acc_i[3], n1);
        if (n2) atomicAdd(&acc_i[4], n2);
        for (int i = tid; i < nd; i += THREADS) {
            const int64_t row = row_at(a.s.dt_order, b.d0 + i, a.s.n_dt);
            int f = 0;
            if (row >= 0 && (shard == 0 || range_shard(a.dts + row * 7) == shard)) {
                const float score = a.scores[row];
                int k = -1;
                for (int q = 0; q < N_CUT; ++q)
                    if (score >= cut[q]) k = q;
                if (k >= 0) {
                    f = 1 | ((k + 1) << 8);
                    atomicAdd(&hist[k], 1);
                }
            }
            dt_flag[i] = f;
        }
    }
    __syncthreads();
    const int n_gt1 = acc_i[3], n_gt2 = acc_i[4];
    for (int64_t p = tid; p < (int64_t)nd * ng; p += THREADS) {
        const int i = (int)(p / ng), j = (int)(p - (int64_t)i * ng);
        if ((dt_flag[i] & 1) && (gt_flag[j] & 1) && weight_of(a.iou, base + p, box, thr) > 0) {
            if (!(dt_flag[i] & 2)) atomicOr(&dt_flag[i], 2);
            if (!(gt_flag[j] & 2)) atomicOr(&gt_flag[j], 2);
        }
    }
    __syncthreads();

    // 2: ordered compaction of the rows and columns with a gated pair
    int nr = 0, nc = 0;
    for (int t0 = 0; t0 < nd; t0 += THREADS) {
        const int i = t0 + tid;
        const int f = i < nd ? dt_flag[i] : 0;
        int total;
        const int rank = tile_rank((f & 3) == 3, nr, wave_count, &total);
        if ((f & 3) == 3) row_pos[rank] = i, row_k[rank] = (signed char)((f >> 8) - 1), u[rank] = 0, col_of[rank] = NONE;
        nr += total;
    }
    for (int t0 = 0; t0 < ng; t0 += THREADS) {
        const int j = t0 + tid;
        const int f = j < ng ? gt_flag[j] : 0;
        int total;
        const int rank = tile_rank((f & 3) == 3, nc, wave_count, &total);
        if ((f & 3) == 3) col_pos[rank] = j, col_lvl[rank] = (unsigned char)(f >> 8), owner[rank] = NONE;
        nc += total;
    }
    __syncthreads();

    // 3: insertion in score order; a count after the last row of every cutoff group
    int v[COLS], minv[COLS];  // potential and running minimum of the columns c * THREADS + tid
#pragma unroll
    for (int c = 0; c < COLS; ++c) v[c] = 0;
    int r = 0, matched = 0, tp1 = 0, tp2 = 0;
    long long h1 = 0, h2 = 0;
    for (int k = N_CUT - 1; k >= 0; --k) {
        bool changed = false;
        while (r < nr && row_k[r] >= k) {  // (uniform: LDS values; at most nr insertions over all k)
            changed = true;
            unsigned used = 0;
#pragma unroll
            for (int c = 0; c < COLS; ++c) minv[c] = BIG;
            int i0 = r, j0 = START, dmin = BIG, dway = START, last = NONE;
            bool closed = false;
            for (int step = 0; step <= nc; ++step) {  // a search takes every column at most once, then ends
                const int u0 = u[i0];
                const int64_t wrow = base + (int64_t)row_pos[i0] * ng;
                int best = BIG, best_col = BIG;
#pragma unroll
                for (int c = 0; c < COLS; ++c) {
                    const int j = c * THREADS + tid;
                    if (j < nc && !(used >> c & 1)) {
                        const int cur = -weight_of(a.iou, wrow + col_pos[j], box, thr) - u0 - v[c];
                        if (cur < minv[c]) minv[c] = cur, way[j] = j0;
                        if (minv[c] < best) best = minv[c], best_col = j;
                    }
                }
                if (-u0 < dmin) dmin = -u0, dway = j0;
                // minimum over the workgroup, ties to the lowest column
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const int ov = __shfl_xor(best, o, 64), oc = __shfl_xor(best_col, o, 64);
                    if (ov < best || (ov == best && oc < best_col)) best = ov, best_col = oc;
                }
                if (lane == 0) red_val[wave] = best, red_col[wave] = best_col;
                __syncthreads();
                best = red_val[0], best_col = red_col[0];
                for (int w = 1; w < WAVES; ++w)
                    if (red_val[w] < best || (red_val[w] == best && red_col[w] < best_col)) best = red_val[w], best_col = red_col[w];
                // "unmatched" wins ties
                const int j1 = best < dmin ? best_col : NONE;
                const int delta = best < dmin ? best : dmin;
#pragma unroll
                for (int c = 0; c < COLS; ++c) {
                    const int j = c * THREADS + tid;
                    if (j < nc) {
                        if (used >> c & 1) u[owner[j]] += delta, v[c] -= delta;
                        else minv[c] -= delta;
                    }
                }
                if (tid == 0) u[r] += delta;
                dmin -= delta;
                const int own = j1 >= 0 ? owner[j1] : NONE;
                if (j1 >= 0 && (j1 & (THREADS - 1)) == tid) used |= 1u << (j1 / THREADS);
                __syncthreads();
                if (j1 < 0 || own < 0) {
                    last = j1, closed = true;
                    break;
                }
                j0 = j1, i0 = own;
            }
            if (tid == 0) {
                if (!closed) atomicAdd(&a.errors[ERR_BOUND], 1);  // (the row stays unmatched)
                else {
                    // hand the columns of the path down: every row on it takes the column the search reached it from
                    int target = last, jc = last >= 0 ? way[last] : dway, hops = 0;
                    for (; hops <= nc; ++hops) {
                        const int rr = jc == START ? r : owner[jc];
                        col_of[rr] = target;
                        if (target >= 0) owner[target] = rr;
                        if (jc == START) break;
                        target = jc, jc = way[jc];
                    }
                    if (hops > nc) atomicAdd(&a.errors[ERR_BOUND], 1);
                }
            }
            __syncthreads();
            ++r;
        }
        if (changed) {
            if (tid < 3) acc_i[tid] = 0;
            if (tid < 2) acc_h[tid] = 0;
            __syncthreads();
            int m = 0, t1 = 0, t2 = 0;
            long long q1 = 0, q2 = 0;
            for (int rr = tid; rr < r; rr += THREADS) {
                const int c = col_of[rr];
                if (c < 0) continue;
                const int lvl = col_lvl[c];
                ++m;
                if (lvl > 2) continue;
                const int64_t d = row_at(a.s.dt_order, b.d0 + row_pos[rr], a.s.n_dt), g = row_at(a.s.gt_order, b.g0 + col_pos[c], a.s.n_gt);
                const long long q = d >= 0 && g >= 0 ? heading_quanta(a.dts[d * 7 + 6], a.gts[g * 7 + 6]) : 0;
                ++t2, q2 += q;
                if (lvl <= 1) ++t1, q1 += q;
            }
            if (m) atomicAdd(&acc_i[0], m);
            if (t1) atomicAdd(&acc_i[1], t1), atomicAdd(&acc_h[0], (unsigned long long)q1);
            if (t2) atomicAdd(&acc_i[2], t2), atomicAdd(&acc_h[1], (unsigned long long)q2);
            __syncthreads();
            matched = acc_i[0], tp1 = acc_i[1], tp2 = acc_i[2], h1 = (long long)acc_h[0], h2 = (long long)acc_h[1];
        }
        if (tid == 0) cnt[k][0] = matched, cnt[k][1] = tp1, cnt[k][2] = tp2, head[k][0] = h1, head[k][1] = h2;
    }
    __syncthreads();

    // 4: rows inserted at a cutoff (with or without a gated pair), then the counts into the global tables
    if (tid == 0) {
        int acc = 0;
        for (int k = N_CUT - 1; k >= 0; --k) acc += hist[k], hist[k] = acc;
    }
    __syncthreads();
    for (int e = tid; e < N_CUT * 2; e += THREADS) {
        const int k = e >> 1, lv = e & 1;
        const long long tp = cnt[k][1 + lv], fp = hist[k] - cnt[k][0], fn = (lv ? n_gt2 : n_gt1) - tp, hd = head[k][lv];
        unsigned long long* t = a.tables + ((((int64_t)box * N_ROWS + brow) * 2 + lv) * N_CUT + k) * 4;
        if (tp) atomicAdd(t, (unsigned long long)tp);
        if (fp > 0) atomicAdd(t + 1, (unsigned long long)fp);
        if (fn > 0) atomicAdd(t + 2, (unsigned long long)fn);
        if (hd) atomicAdd(t + 3, (unsigned long long)hd);
    }
}

// ---------------------------------------------------------------------------------------
// AP / APH
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void waymo_summary_kernel(const long long* tables, double* out) {
    __shared__ double prec[2][N_CUT], rec[2][N_CUT];
    const int box = blockIdx.x / RV_WAYMO_NUM_RESULT_ROWS, row = blockIdx.x % RV_WAYMO_NUM_RESULT_ROWS, k = threadIdx.x;
    // result row -> (breakdown row, level): 4 types x 2 levels over all ranges, then per type 3 ranges x 2 levels
    const int brow = row < 8 ? row / 2 : 4 + (row - 8) / 2, lv = row & 1;
    if (k < N_CUT) {
        const long long* t = tables + ((((int64_t)box * N_ROWS + brow) * 2 + lv) * N_CUT + k) * 4;
        const double tp = (double)t[0], fp = (double)t[1], fn = (double)t[2], hd = (double)t[3] * (1.0 / 1099511627776.0);
        prec[0][k] = tp + fp > 0. ? tp / (tp + fp) : 0., rec[0][k] = tp + fn > 0. ? tp / (tp + fn) : 0.;
        prec[1][k] = tp + fp > 0. ? hd / (tp + fp) : 0., rec[1][k] = tp + fn > 0. ? hd / (tp + fn) : 0.;
    }
    __syncthreads();
    if (k < 2) {  // AP, APH
        double top = 0.;  // precision made non-increasing towards higher recall: running maximum from the lowest cutoff up
        for (int q = 0; q < N_CUT; ++q) {
            top = prec[k][q] > top ? prec[k][q] : top;
            prec[k][q] = top;
        }
        double area = 0., before = 0.;
        for (int q = N_CUT - 1; q >= 0; --q) {
            area += (rec[k][q] - before) * prec[k][q];
            before = rec[k][q];
        }
        out[((int64_t)box * RV_WAYMO_NUM_RESULT_ROWS + row) * 2 + k] = area;
    }
}

int64_t pair_capacity(int64_t n_dt, int64_t n_gt) { return n_dt * (n_gt < RV_WAYMO_MAX_GTS ? n_gt : RV_WAYMO_MAX_GTS); }

}  // namespace

extern "C" int64_t rv_waymo_match_workspace_bytes(int64_t n_dt, int64_t n_gt, int32_t n_segments) {
    if (n_dt < 0 || n_gt < 0 || n_segments < 1) return 0;
    return rv_align256(((int64_t)n_segments + 1) * 8) + rv_align256(pair_capacity(n_dt, n_gt) * 8) + 256;
}

extern "C" int rv_waymo_iou(const float* dts, const int64_t* dt_order, const int64_t* dt_offsets, int64_t n_dt, const float* gts,
                            const int64_t* gt_order, const int64_t* gt_offsets, int64_t n_gt, int32_t n_segments, void* workspace,
                            rvStream stream) {
    RV_REQUIRE(n_dt >= 0 && n_gt >= 0 && n_dt <= 0x7fffffff && n_gt <= 0x7fffffff, "rv_waymo_iou: n_dt = %lld, n_gt = %lld", (long long)n_dt,
               (long long)n_gt);
    RV_REQUIRE(n_segments >= 1, "rv_waymo_iou: %d segments", n_segments);
    RV_REQUIRE(dt_offsets && gt_offsets && workspace, "rv_waymo_iou: null segment offsets or workspace");
    RV_REQUIRE((uintptr_t)workspace % 8 == 0, "rv_waymo_iou: workspace must be 8-byte aligned");
    RV_REQUIRE(n_dt == 0 || (dts && dt_order), "rv_waymo_iou: null detection buffer");
    RV_REQUIRE(n_gt == 0 || (gts && gt_order), "rv_waymo_iou: null ground-truth buffer");
    Segments s = {dt_order, dt_offsets, gt_order, gt_offsets, n_dt, n_gt};
    int64_t* pair_off = (int64_t*)workspace;
    float2* iou = (float2*)((char*)workspace + rv_align256(((int64_t)n_segments + 1) * 8));
    const int64_t capacity = pair_capacity(n_dt, n_gt);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(waymo_offsets_kernel, dim3(1), dim3(THREADS), 0, st, s, n_segments, pair_off);
    const int64_t blocks = (capacity + THREADS - 1) / THREADS;
    if (blocks > 0)
        hipLaunchKernelGGL(waymo_iou_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(THREADS), 0, st, s, dts, gts, n_segments,
                           pair_off, capacity, iou);
    RV_CHECK_LAUNCH("waymo_iou_kernel");
    return 0;
}

extern "C" int rv_waymo_match(const float* dts, const float* scores, const int64_t* dt_order, const int64_t* dt_offsets, int64_t n_dt,
                              const float* gts, const uint8_t* gt_level, const int64_t* gt_order, const int64_t* gt_offsets, int64_t n_gt,
                              const uint8_t* sweep_valid, int32_t n_sweeps, const float* host_iou_thresholds, const void* workspace,
                              int64_t* tables, int32_t* errors, rvStream stream) {
    RV_REQUIRE(n_dt >= 0 && n_gt >= 0 && n_dt <= 0x7fffffff && n_gt <= 0x7fffffff, "rv_waymo_match: n_dt = %lld, n_gt = %lld", (long long)n_dt,
               (long long)n_gt);
    RV_REQUIRE(n_sweeps >= 1 && n_sweeps <= RV_WAYMO_MAX_SWEEPS, "rv_waymo_match: %d sweeps (1 .. %d)", n_sweeps, RV_WAYMO_MAX_SWEEPS);
    RV_REQUIRE(dt_offsets && gt_offsets && workspace && tables && errors && host_iou_thresholds, "rv_waymo_match: null argument");
    RV_REQUIRE((uintptr_t)workspace % 8 == 0, "rv_waymo_match: workspace must be 8-byte aligned");
    RV_REQUIRE(n_dt == 0 || (dts && scores && dt_order), "rv_waymo_match: null detection buffer");
    RV_REQUIRE(n_gt == 0 || (gts && gt_level && gt_order), "rv_waymo_match: null ground-truth buffer");
    WaymoMatchArgs a;
    memset(&a, 0, sizeof(a));
    for (int t = 0; t < 5; ++t) {
        RV_REQUIRE(host_iou_thresholds[t] >= 0.f && host_iou_thresholds[t] <= 1.f, "rv_waymo_match: IoU threshold %d is %g", t,
                   (double)host_iou_thresholds[t]);
        a.thr[t] = host_iou_thresholds[t];
    }
    const int n_segments = n_sweeps * 4;
    a.s = Segments{dt_order, dt_offsets, gt_order, gt_offsets, n_dt, n_gt};
    a.dts = dts, a.scores = scores, a.gts = gts, a.gt_level = gt_level, a.sweep_valid = sweep_valid;
    a.pair_off = (const int64_t*)workspace;
    a.iou = (const float*)((const char*)workspace + rv_align256(((int64_t)n_segments + 1) * 8));
    a.capacity = pair_capacity(n_dt, n_gt);
    a.tables = (unsigned long long*)tables, a.errors = errors;
    hipLaunchKernelGGL(waymo_match_kernel, dim3((unsigned)n_segments * 8), dim3(THREADS), 0, (hipStream_t)stream, a);
    RV_CHECK_LAUNCH("waymo_match_kernel");
    return 0;
}

extern "C" int rv_waymo_summarize(const int64_t* tables, double* out, rvStream stream) {
    RV_REQUIRE(tables && out, "rv_waymo_summarize: null argument");
    hipLaunchKernelGGL(waymo_summary_kernel, dim3(2 * RV_WAYMO_NUM_RESULT_ROWS), dim3(128), 0, (hipStream_t)stream, (const long long*)tables,
                       out);
    RV_CHECK_LAUNCH("waymo_summary_kernel");
    return 0;
}
