// What the list path (nms.hip) and the batch path (nms2.hip) share: the pair masks of one row box against a 64-box column tile, the
// suppression scan of one mask word, the weighted sum over one kept box's cluster (semantics: oracle/nms.py).  The kernels keep what
// differs: where rows and tiles are loaded from, how a mask word is addressed, where "kept" is recorded.
#pragma once
#include "nms_geom.h"

namespace {

// 64 boxes of one column block: [x1, y1, x2, y2, ry, fp32(sin ry), fp32(cos ry)] and the class ids
struct ColTile {
    float box[64][7];
    int32_t cat[64];
};

// The weighted-NMS choices of a call (RV_WNMS_* of include/rv3d.h; 0 = the declaration of oracle/nms.py).  They travel as a kernel
// argument, so every branch on them is wave-uniform.  Where each one lives: the two comparisons in pair_bits, the alive mask in
// scan_diagonal / scan_fold, the score column after cluster_sum (the kernels' store).
constexpr int kWnmsMergeSuppressed = RV_WNMS_MERGE_SUPPRESSED, kWnmsScoreKeeper = RV_WNMS_SCORE_KEEPER, kWnmsNmsGe = RV_WNMS_NMS_GE,
              kWnmsMergeGe = RV_WNMS_MERGE_GE, kWnmsAll = 15;

// Bits j of the column block at j0 (`jn` boxes in the tile: wave-uniform, so the loop is scalar) whose IoU with row box i passes the
// threshold tests (`>`; `>=` under kWnmsNmsGe / kWnmsMergeGe); only later boxes (i < j0 + j < end) of the same class are tested.
// HARD: the suppression mask only (merge_t is not read, bits_m stays 0; flags = 0).
template <bool HARD>
__device__ __forceinline__ void pair_bits(const ColTile& tile, int jn, const float* a, float sa, float ca, int32_t cat_i, int64_t i,
                                          int64_t j0, int64_t end, float nms_t, float merge_t, int flags, unsigned long long& bits_n,
                                          unsigned long long& bits_m) {
    // bounding circle of box i: boxes whose circles are apart cannot intersect -- their IoU is 0 in the clipping arithmetic
    // too, so skipping them changes no bit of the masks as long as an IoU of 0 fails both tests: `0 > t` fails for t >= 0,
    // `0 >= t` only for t > 0 -- a `>=` test against a threshold of 0 lets every far pair pass, and such a call tests them all.
    // Skips ~all pairs of a spread-out scene.
    const bool nms_ge = !HARD && (flags & kWnmsNmsGe), merge_ge = !HARD && (flags & kWnmsMergeGe);
    const float cxi = 0.5f * (a[0] + a[2]), cyi = 0.5f * (a[1] + a[3]);
    const float ri = 0.5f * sqrtf((a[2] - a[0]) * (a[2] - a[0]) + (a[3] - a[1]) * (a[3] - a[1]));
    const bool skip_far = (nms_ge ? nms_t > 0.f : nms_t >= 0.f) && (HARD || (merge_ge ? merge_t > 0.f : merge_t >= 0.f));
    bits_n = bits_m = 0ull;
    for (int j = 0; j < jn; ++j) {
        const float* b = tile.box[j];
        if (j0 + j <= i || tile.cat[j] != cat_i || j0 + j >= end) continue;
        const float dx = 0.5f * (b[0] + b[2]) - cxi, dy = 0.5f * (b[1] + b[3]) - cyi;
        const float rj = 0.5f * sqrtf((b[2] - b[0]) * (b[2] - b[0]) + (b[3] - b[1]) * (b[3] - b[1]));
        if (skip_far && dx * dx + dy * dy > (ri + rj) * (ri + rj) * 1.001f + 1e-4f) continue;
        const float iou = rotated_iou(a, sa, ca, b, b[5], b[6]);
        if (iou > nms_t || (nms_ge && iou == nms_t)) bits_n |= 1ull << j;
        if constexpr (!HARD)
            if (iou > merge_t || (merge_ge && iou == merge_t)) bits_m |= 1ull << j;
    }
}

// The chain "is box q of this block still alive?" over one mask word, resolved by ONE wave (all 64 lanes call this) from the diagonal
// words held one per lane: 64 register-only steps, lane q's word through readlane.  `in_bits`: the lanes that hold a box; `rem`: the
// boxes of the block suppressed so far, updated; `kept`: the boxes of the block that stay; `alive_mine` (weighted only): the boxes not
// suppressed when this lane's box was visited, for a kept box -- every box under `merge_all` (kWnmsMergeSuppressed: a cluster takes
// suppressed boxes too).
template <bool HARD>
__device__ __forceinline__ void scan_diagonal(unsigned long long diag, unsigned long long in_bits, int lane, bool merge_all,
                                              unsigned long long& rem, unsigned long long& kept, unsigned long long& alive_mine) {
    const uint32_t dlo = (uint32_t)diag, dhi = (uint32_t)(diag >> 32);
    kept = alive_mine = 0ull;
    for (int q = 0; q < 64; ++q) {  // uniform loop
        if (!((in_bits >> q) & 1ull) || ((rem >> q) & 1ull)) continue;
        kept |= 1ull << q;
        if constexpr (!HARD)
            if (lane == q) alive_mine = merge_all ? ~0ull : ~rem;
        rem |= ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)dhi, q) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)dlo, q);
    }
}

// A later word of the block's kept boxes, in visiting order: the merge row of each loses the boxes suppressed before its visit (not
// under `merge_all`: the row stays as pair_bits wrote it), then its suppression row joins `r`.  `word(q)`: index of that word of box q
// of the block, in both masks.  HARD: one read of nms_mask.
template <bool HARD, class Word>
__device__ __forceinline__ unsigned long long scan_fold(unsigned long long r, unsigned long long kept, bool merge_all,
                                                        const unsigned long long* nms_mask, unsigned long long* merge_mask, Word word) {
    while (kept) {
        const int q = __ffsll((long long)kept) - 1;
        kept &= kept - 1;
        const int64_t mw = word(q);
        if constexpr (!HARD)
            if (!merge_all) merge_mask[mw] &= ~r;
        r |= nms_mask[mw];
    }
    return r;
}

// Weighted sum of column c (lane; idle at c >= d) of `data` (rows of d floats, the last one the weight) over the cluster of kept box i:
// the box itself, then the members named by the merge words w_first .. w_last (`word(w)`) in ascending index order -- a fixed order.
// The caller stores acc / wsum; under kWnmsScoreKeeper the last column takes the kept box's own weight instead (the sums are the same).
template <class Word>
__device__ __forceinline__ void cluster_sum(const float* data, int d, int c, int64_t i, int w_first, int w_last, Word word, float& acc,
                                            float& wsum, long long& members) {
    const bool active = c < d;
    const float wi = data[i * d + d - 1];
    acc = active ? wi * data[i * d + c] : 0.f;
    wsum = wi;
    members = 1;
    for (int w = w_first; w <= w_last; ++w) {
        unsigned long long bits = word(w);
        while (bits) {
            const int b = __ffsll((long long)bits) - 1;
            bits &= bits - 1;
            const int64_t j = (int64_t)w * 64 + b;
            const float wj = data[j * d + d - 1];
            if (active) acc += wj * data[j * d + c];
            wsum += wj;
            ++members;
        }
    }
}

}  // namespace
