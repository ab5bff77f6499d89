// nms.hip -- weighted NMS on device; replaces `weighted_nms_ext.wnms_gpu` (math/ops/nms.py:161-170).
//
// The third-party kernel's arithmetic is not in the reference tree (parity unpinned); this
// file implements the semantics declared in oracle/nms.py and matches oracle/c/oracle.c bit for
// bit (compiled with -ffp-contract=off; IEEE division; sin/cos of the yaw are fp32 roundings of
// the fp64 values).  Three stages, all wavefront-level integer/bit work:
//   1. pairwise rotated-BEV-IoU bit masks (upper triangle): one 64-lane wave = 64 boxes x one
//      64-box column block staged in LDS; two u64 words per lane (IoU > nms, IoU > merge);
//   2. the inherently sequential scan over boxes in score order: one workgroup keeps the
//      suppressed-set bit vector in LDS; per kept box it ORs one mask row into it and masks the
//      merge row with the boxes still alive (=> cluster membership);
//   3. cluster merge: one wave per kept box, lanes = data columns, members visited in ascending
//      index order (fixed summation order => reproducible).
// Hard NMS (`rv_nms_rotated`: detectron2's `nms_rotated` on a score-sorted list, math/ops/nms.py:40-44) is stages 1 and 2
// with the mode as a template parameter: one mask (IoU > iou_threshold), a scan that reads it and writes `keep`, no stage 3.
// The declaration's four free choices (merge set, score column, `>` or `>=` in the two tests) are flags of rv_wnms_opt (RV_WNMS_*,
// include/rv3d.h): a kernel argument, read where nms_core.h makes the choice; rv_wnms / rv_wnms_classes are rv_wnms_opt with 0.
// The pair loop of stage 1, the word scan of stage 2 and the cluster sum of stage 3 are nms_core.h's, shared with the batch path
// (nms2.hip); the kernels here load rows and tiles from the caller's list and address the masks as dense [n][cb] words.
#include "common.h"
#include "nms_core.h"

namespace {

__global__ void sincos_kernel(const float* boxes, int64_t n, float* sc) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        yaw_sincos(boxes[i * 5 + 4], sc[2 * i], sc[2 * i + 1]);
}

// grid (col_block, row_block); only col_block >= row_block does work
// cats (optional): class id per box -- boxes of different classes neither suppress nor merge (all classes of a sweep in
// one launch instead of the reference's per-class loop)
// HARD: the suppression mask only (merge_t / merge_mask are not read)
template <bool HARD>
__global__ __launch_bounds__(64) void iou_mask_kernel(const float* boxes, const float* sc, const int32_t* cats, int64_t n, int cb,
                                                      float nms_t, float merge_t, int flags, unsigned long long* nms_mask,
                                                      unsigned long long* merge_mask) {
    const int col = blockIdx.x, row = blockIdx.y;
    if (col < row) return;
    __shared__ ColTile tile;
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)col * 64;
    if (j0 + t < n) {
        tile.cat[t] = cats ? cats[j0 + t] : 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) tile.box[t][k] = boxes[(j0 + t) * 5 + k];
        tile.box[t][5] = sc[2 * (j0 + t)];
        tile.box[t][6] = sc[2 * (j0 + t) + 1];
    }
    __syncthreads();
    const int64_t i = (int64_t)row * 64 + t;
    if (i >= n) return;
    float a[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) a[k] = boxes[i * 5 + k];
    const float sa = sc[2 * i], ca = sc[2 * i + 1];
    const int32_t cat_i = cats ? cats[i] : 0;
    unsigned long long bits_n, bits_m;
    pair_bits<HARD>(tile, (int)(n - j0 < 64 ? n - j0 : 64), a, sa, ca, cat_i, i, j0, n, nms_t, merge_t, flags, bits_n, bits_m);
    nms_mask[i * cb + col] = bits_n;
    if constexpr (!HARD) merge_mask[i * cb + col] = bits_m;
}

// One workgroup; remv (suppressed set) lives in LDS.  The scan walks the boxes in blocks of 64 (one mask word): one wave resolves
// the block (scan_diagonal), then every thread owning a later word w folds the rows of the block's kept boxes into remv[w]
// (scan_fold) -- one round of global loads and two barriers per 64 boxes instead of per kept box.  Same visiting order and the
// same sets as the box-by-box loop (oracle/nms.py).
template <bool HARD>
__global__ __launch_bounds__(1024) void scan_kernel(int64_t n, int cb, int flags, const unsigned long long* nms_mask,
                                                    unsigned long long* merge_mask, long long* keep, long long* num_out) {
    extern __shared__ unsigned long long remv[];
    __shared__ unsigned long long kept_word;
    const bool merge_all = !HARD && (flags & kWnmsMergeSuppressed);
    for (int w = threadIdx.x; w < cb; w += blockDim.x) remv[w] = 0ull;
    __syncthreads();
    long long kept_total = 0;
    for (int wi = 0; wi < cb; ++wi) {
        if (threadIdx.x < 64) {
            const int b = threadIdx.x;
            const int64_t i = (int64_t)wi * 64 + b;
            const bool in = i < n;
            const unsigned long long diag = in ? nms_mask[i * cb + wi] : 0ull;
            unsigned long long rem = remv[wi], kept, alive_mine;
            scan_diagonal<HARD>(diag, __ballot(in), b, merge_all, rem, kept, alive_mine);
            if ((kept >> b) & 1ull) {
                keep[kept_total + __popcll(kept & ((1ull << b) - 1ull))] = i;
                // cluster = merge candidates not suppressed before i was visited (merge_all: all of them)
                if constexpr (!HARD)
                    if (!merge_all) merge_mask[i * cb + wi] &= alive_mine;
            }
            if (b == 0) {
                remv[wi] = rem;
                kept_word = kept;
            }
        }
        __syncthreads();
        const unsigned long long kept = kept_word;
        kept_total += __popcll(kept);
        for (int w = wi + 1 + threadIdx.x; w < cb; w += blockDim.x)
            remv[w] = scan_fold<HARD>(remv[w], kept, merge_all, nms_mask, merge_mask, [&](int q) { return ((int64_t)wi * 64 + q) * cb + w; });
        __syncthreads();
    }
    if (threadIdx.x == 0) *num_out = kept_total;
}

// one wave per kept box; lane = data column
__global__ __launch_bounds__(64) void merge_kernel(const float* data, int d, int cb, int flags, const unsigned long long* merge_mask,
                                                   const long long* keep, const long long* num_out, float* output,
                                                   long long* count) {
    const long long o = blockIdx.x;
    if (o >= *num_out) return;
    const long long i = keep[o];
    const int c = threadIdx.x;
    float acc, wsum;
    long long members;
    cluster_sum(data, d, c, i, (int)(i >> 6), cb - 1, [&](int w) { return merge_mask[i * cb + w]; }, acc, wsum, members);
    if (c < d) output[o * d + c] = (flags & kWnmsScoreKeeper) && c == d - 1 ? data[i * d + c] : acc / wsum;
    if (c == 0) count[o] = members;
}

__global__ void pairwise_iou_kernel(const float* a, int64_t n, const float* b, int64_t m, float* out) {
    const int64_t total = n * m;
    for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = k / m, j = k - i * m;
        float sa, ca, sb, cb;
        yaw_sincos(a[i * 5 + 4], sa, ca);
        yaw_sincos(b[j * 5 + 4], sb, cb);
        out[k] = rotated_iou(a + i * 5, sa, ca, b + j * 5, sb, cb);
    }
}

// workspace of one list, byte offsets: nms_mask [n][cb] at 0, merge_mask [n][cb] (weighted only), sc [n][2], num_out
struct ListLayout {
    int64_t merge_mask, sc, num_out, bytes;
};
ListLayout carve_list(int64_t n, bool hard) {
    const int64_t mask = rv_align256(n * ((n + 63) / 64) * 8);
    ListLayout l;
    l.merge_mask = mask;
    l.sc = hard ? mask : 2 * mask;
    l.num_out = l.sc + rv_align256(n * 2 * 4);
    l.bytes = l.num_out + 256;
    return l;
}

// HARD: `data`, `output`, `count`, `merge_thresh` and `flags` (0) are not used
template <bool HARD>
int launch_list(const char* who, const float* boxes, const float* data, const int32_t* cats, int64_t n, int32_t d, float nms_thresh,
                float merge_thresh, int32_t flags, float* output, int64_t* keep, int64_t* count, void* workspace, int64_t* host_num_out, rvStream stream) {
    RV_REQUIRE(host_num_out, "%s: null host_num_out", who);
    *host_num_out = 0;
    RV_REQUIRE((flags & ~kWnmsAll) == 0, "%s: unknown flag bits 0x%x (RV_WNMS_*: 0x%x)", who, (unsigned)(flags & ~kWnmsAll), (unsigned)kWnmsAll);
    if (n == 0) return 0;
    RV_REQUIRE(boxes && keep && workspace && (HARD || (data && output && count)), "%s: null argument", who);
    RV_REQUIRE(HARD || (d >= 1 && d <= 64), "%s: data width %d unsupported (1..64)", who, d);
    const int64_t cb64 = (n + 63) / 64;
    RV_REQUIRE(cb64 * 8 <= 160 * 1024 - 256, "%s: too many boxes (%lld)", who, (long long)n);
    const int cb = (int)cb64;
    hipStream_t st = (hipStream_t)stream;
    const ListLayout l = carve_list(n, HARD);
    uint8_t* ws = (uint8_t*)workspace;
    unsigned long long* nms_mask = (unsigned long long*)ws;
    unsigned long long* merge_mask = HARD ? nullptr : (unsigned long long*)(ws + l.merge_mask);
    float* sc = (float*)(ws + l.sc);
    long long* num_out = (long long*)(ws + l.num_out);
    hipLaunchKernelGGL(sincos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, boxes, n, sc);
    hipLaunchKernelGGL(iou_mask_kernel<HARD>, dim3(cb, cb), dim3(64), 0, st, boxes, sc, cats, n, cb, nms_thresh, merge_thresh, (int)flags,
                       nms_mask, merge_mask);
    RV_LDS_OPT_IN(160 * 1024 - 256, scan_kernel<HARD>);  // + the static word
    hipLaunchKernelGGL(scan_kernel<HARD>, dim3(1), dim3(cb < 1024 ? ((cb + 63) / 64) * 64 : 1024), (size_t)cb * 8, st, n, cb, (int)flags,
                       nms_mask, merge_mask, (long long*)keep, num_out);
    if constexpr (!HARD)
        hipLaunchKernelGGL(merge_kernel, dim3((unsigned)n), dim3(64), 0, st, data, d, cb, (int)flags, merge_mask, (const long long*)keep,
                           num_out, output, (long long*)count);
    RV_CHECK_LAUNCH(HARD ? "nms_rotated kernels" : "wnms kernels");
    long long host = 0;
    hipError_t e = hipMemcpyAsync(&host, num_out, sizeof(host), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) RV_FAIL("%s: %s", who, hipGetErrorString(e));
    *host_num_out = host;
    return 0;
}

}  // namespace

extern "C" int64_t rv_wnms_workspace_bytes(int64_t n) { return carve_list(n, false).bytes; }
extern "C" int64_t rv_nms_rotated_workspace_bytes(int64_t n) { return carve_list(n, true).bytes; }

extern "C" int rv_wnms(const float* boxes, const float* data, int64_t n, int32_t d, float nms_thresh, float merge_thresh,
                       float* output, int64_t* keep, int64_t* count, void* workspace, int64_t* host_num_out,
                       rvStream stream) {
    return rv_wnms_opt(boxes, data, nullptr, n, d, nms_thresh, merge_thresh, output, keep, count, workspace, host_num_out, stream, 0);
}

extern "C" int rv_wnms_classes(const float* boxes, const float* data, const int32_t* cats, int64_t n, int32_t d, float nms_thresh,
                               float merge_thresh, float* output, int64_t* keep, int64_t* count, void* workspace,
                               int64_t* host_num_out, rvStream stream) {
    return rv_wnms_opt(boxes, data, cats, n, d, nms_thresh, merge_thresh, output, keep, count, workspace, host_num_out, stream, 0);
}

extern "C" int rv_wnms_opt(const float* boxes, const float* data, const int32_t* cats, int64_t n, int32_t d, float nms_thresh,
                           float merge_thresh, float* output, int64_t* keep, int64_t* count, void* workspace, int64_t* host_num_out,
                           rvStream stream, int32_t flags) {
    return launch_list<false>("rv_wnms", boxes, data, cats, n, d, nms_thresh, merge_thresh, flags, output, keep, count, workspace,
                              host_num_out, stream);
}

extern "C" int rv_nms_rotated(const float* boxes, const int32_t* cats, int64_t n, float iou_threshold, int64_t* keep, void* workspace,
                              int64_t* host_num_out, rvStream stream) {
    return launch_list<true>("rv_nms_rotated", boxes, nullptr, cats, n, 0, iou_threshold, 0.f, 0, nullptr, keep, nullptr, workspace,
                             host_num_out, stream);
}

extern "C" int rv_rotated_iou(const float* a, int64_t n, const float* b, int64_t m, float* out, rvStream stream) {
    if (n * m == 0) return 0;
    RV_REQUIRE(a && b && out, "rv_rotated_iou: null argument");
    const int64_t blocks = (n * m + 255) / 256;
    hipLaunchKernelGGL(pairwise_iou_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                       a, n, b, m, out);
    RV_CHECK_LAUNCH("pairwise_iou_kernel");
    return 0;
}
