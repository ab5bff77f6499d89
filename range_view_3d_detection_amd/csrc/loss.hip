// loss.hip -- fused detection loss (forward reductions + analytic gradients), one thread per pixel.
//
// Reference: compute_classification_targets with GAUSSIAN affinity, k = inf, normalize_affinities =
// false (math/ops/assignment.py:76-161 -- the per-instance python loop reduces to a per-pixel map),
// varifocal_loss (nn/functional/__init__.py:8-27), DetectionHead.compute_*_loss and
// reduce_multiscale_loss (nn/heads/detection_head.py:309-449).  HBM-bound element-wise work:
// reads (n_cls + 8) logits/regressands + 3 + 8 + a few labels per pixel, writes the same number of
// gradients.  Reductions: registers -> wave shuffles -> one fp64 atomic per wave and quantity.
//
//   sums[0] = sum w_cls * VFL * mask            sums[1] = ... * foreground      sums[2] = ... * background
//   sums[3] = number of foreground pixels       sums[4..11] = sum of the un-normalised regression terms
//   sums[12] = max(total_objects, 1)            sums[13] = sums[3] + smoothing (total_fg)
// loss = sums[0]/sums[13] + (sums[4]+..+sums[11])/sums[12]   (assembled by the host wrapper, on device).
// Several (level, task) entries: one row of RV_LOSS_SUMS_LEN sums per entry, filled by ONE launch over an entry table, then
// loss_table_finish_kernel normalises every row by the foreground / object counts of ALL rows (reduce_multiscale_loss, :379-449).
#include "common.h"

namespace {

struct LossArgs {
    const float* logits;  // NHWC, ld_logits
    const float* reg;     // NHWC, ld_reg
    const float* cart;    // NCHW (B,3,H,W)
    const uint8_t* mask;  // (B,H,W)
    const int64_t* labels;
    const int64_t* panoptics;
    const float* reg_targets;  // NCHW (B,8,H,W)
    const int64_t* ppo;
    const int32_t* num_objects;
    int B, n_cls, H, W, ld_logits, ld_reg;
    float coding[8];
    float cls_w, reg_w, smoothing, sigma, alpha, gamma;
    int az_inv;
    double* sums;
    float* soft;  // optional NCHW (B,n_cls,H,W)
    float* fg;    // optional (B,H,W)
    float* d_logits;
    float* d_reg;
    float grad_scale;
};

// centre of decode_range_view: fp64 arithmetic rounded to fp32 (math/ops/coding.py:126-144)
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

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// ---- loss kinds (rvLossKinds, include/rv3d.h): the per-element terms of the table pair.  alpha / gamma / the kinds are wave-uniform. ----
// b^gamma without powf for the small integers
__device__ __forceinline__ float pow_gamma(float b, float g) {
    return g == 2.f ? b * b : (g == 1.f ? b : (g == 3.f ? b * b * b : (g == 0.f ? 1.f : powf(b, g))));
}
// gamma * b^(gamma - 1): the factor of d/dx b^gamma (gamma == 0: exactly 0, also at b == 0)
__device__ __forceinline__ float dpow_gamma(float b, float g) {
    return g == 2.f ? 2.f * b : (g == 1.f ? 1.f : (g == 3.f ? 3.f * (b * b) : (g == 0.f ? 0.f : g * powf(b, g - 1.f))));
}

// One class logit x with soft target t: the loss (BACKWARD == false) or d loss / d x.  One exponential serves sigmoid(x), sigmoid(-x) =
// 1 - p (the other branch of the same select: never a subtraction) and both softplus values.
template <int CLS, bool BACKWARD>
__device__ __forceinline__ float cls_term(float x, float t, float alpha, float gamma) {
    const float e = expf(-fabsf(x));
    const float p = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    const float sp = fmaxf(x, 0.f) + log1pf(e);
    if (CLS == RV_CLS_VARIFOCAL) {  // (the text of the default path below: the same numbers)
        const float pg = gamma == 2.f ? p * p : powf(p, gamma);
        if (!BACKWARD) {
            const float bce = sp - x * t;
            return t > 0.f ? t * bce : alpha * pg * bce;
        }
        return t > 0.f ? t * (p - t) : alpha * pg * (gamma * (1.f - p) * sp + p);
    }
    const float np = x >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);  // 1 - p
    const float bce = sp - x * t;
    if (CLS == RV_CLS_FOCAL) {
        const float q = p * (1.f - t) + np * t;
        const float at = alpha < 0.f ? 1.f : alpha * t + (1.f - alpha) * (1.f - t);
        if (!BACKWARD) return at * pow_gamma(q, gamma) * bce;
        return at * (dpow_gamma(q, gamma) * (p * np) * (1.f - 2.f * t) * bce + pow_gamma(q, gamma) * (p - t));
    }
    // RV_CLS_PENALTY_REDUCED: at t == 1 bce = softplus(x) - x = softplus(-x), formed without the cancellation
    const float spn = fmaxf(-x, 0.f) + log1pf(e);
    const float w = 1.f - t, w2 = w * w, w4 = w2 * w2;
    const float pg = pow_gamma(p, gamma), npg = pow_gamma(np, gamma);
    if (!BACKWARD) return (t == 1.f ? npg * spn : 0.f) + alpha * w4 * pg * bce;
    return (t == 1.f ? -(npg * (gamma * p * spn + np)) : 0.f) + alpha * w4 * pg * (gamma * np * bce + (p - t));
}

// One regressand residual d = r - t: the element-wise loss, or its derivative (both before reg_weight).
template <bool BACKWARD>
__device__ __forceinline__ float reg_term(int kind, float param, float d) {
    const float ad = fabsf(d);
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    switch (kind) {
        case RV_REG_SMOOTH_L1:  // (beta == 0: the comparison is never true -> L1, as torch defines it)
            if (!BACKWARD) return ad < param ? 0.5f * d * d / param : ad - 0.5f * param;
            return ad < param ? d / param : sgn;
        case RV_REG_HUBER:
            if (!BACKWARD) return ad <= param ? 0.5f * d * d : param * (ad - 0.5f * param);
            return ad <= param ? d : param * sgn;
        case RV_REG_MSE:
            return BACKWARD ? 2.f * d : d * d;
        default:
            return BACKWARD ? sgn : ad;
    }
}

// The work of workgroup `block` of `n_blocks` on one (level, task): shared by the one-level kernel and the entry-table kernel, which
// differ only in where a workgroup finds its tensors.  total_fg / total_obj / gscale are read by the caller (BACKWARD only).
// AFF_MAP: the pixel's affinity is read from `aff_map` (B,H,W), which rv_soft_assign filled (softassign.hip: BEV affinity,
// normalize_affinities, finite k), instead of being the per-pixel exponential below.
// CLS: -1 = the default recipe (varifocal + L1, the text below as it always was); RV_CLS_* = the loss kinds of the table pair:
// cls_term per class, reg_term(reg_kind, reg_param: beta / delta) per regressand.  Everything else -- affinity, foreground, normalisers, reductions -- is shared.
template <bool BACKWARD, bool AFF_MAP = false, int CLS = -1>
__device__ __forceinline__ void loss_tile(const LossArgs& a, int64_t block, int64_t n_blocks, double total_fg, double total_obj, float gscale,
                                          const float* aff_map = nullptr, int reg_kind = RV_REG_L1, float reg_param = 0.f) {
    const int64_t hw = (int64_t)a.H * a.W, total = (int64_t)a.B * hw;
    double acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0.0;
    for (int64_t i = block * (int64_t)blockDim.x + threadIdx.x; i < total; i += n_blocks * blockDim.x) {
        const int64_t b = i / hw, pix = i - b * hw;
        const float m = a.mask[i] ? 1.f : 0.f;
        const float* cart = a.cart + b * 3 * hw;
        const float px = cart[pix], py = cart[hw + pix], pz = cart[2 * hw + pix];
        float r[8], tg[8];
        {  // (rows are 128-byte aligned: stored channel counts are multiples of 32 -- two 16-byte loads instead of eight 4-byte ones)
            const f32x4 r0 = *(const f32x4*)(a.reg + i * a.ld_reg), r1 = *(const f32x4*)(a.reg + i * a.ld_reg + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r[j] = r0[j];
                r[4 + j] = r1[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) tg[j] = a.reg_targets[(b * 8 + j) * hw + pix];
        const int64_t label = a.labels[i];
        const bool inst = a.panoptics[i] > 0;
        float aff = 0.f;
        if (AFF_MAP) {
            aff = aff_map[i];
        } else if (inst) {
            float cp[3], cg[3];
            decode_centre(r, px, py, pz, 1, cp);  // predictions are always decoded azimuth-invariantly (assignment.py:112)
            decode_centre(tg, px, py, pz, a.az_inv, cg);
            const float dx = cp[0] - cg[0], dy = cp[1] - cg[1], dz = cp[2] - cg[2];
            aff = expf(-sqrtf(dx * dx + dy * dy + dz * dz) / (a.sigma * a.sigma));
        }
        const bool fg = aff != 0.f;
        const bool bg = !fg && m != 0.f;
        if (!BACKWARD && a.fg) a.fg[i] = fg ? 1.f : 0.f;
        // ---- classification: varifocal loss over the classes ----
        float cls_sum = 0.f;
        // A thread reads its pixel's logits: with 4-byte loads that is n_cls instructions of 64 lanes x 4 bytes, every lane on a
        // line of its own (128-byte rows), and the same again for the gradient stores -- the rows thrash the 32 KB L1 and the
        // kernel spent its time re-fetching lines.  Rows of 32 floats (the rv-* recipes: 26 / 3 classes) go through eight
        // 16-byte loads / stores and a fully unrolled class loop instead.
        const bool row32 = a.ld_logits == 32;
        f32x4 lv[8], gv[8];
        if (row32) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                lv[q] = *(const f32x4*)(a.logits + i * 32 + q * 4);
                gv[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int c = 0; c < 32; ++c) {
            if (c >= (row32 ? a.n_cls : 0)) break;
            const float x = lv[c >> 2][c & 3];
            const float t = (label == c) ? aff : 0.f;
            if (!BACKWARD && a.soft) a.soft[(b * a.n_cls + c) * hw + pix] = t;
            if (CLS >= 0) {
                const float v = cls_term<(CLS < 0 ? 0 : CLS), BACKWARD>(x, t, a.alpha, a.gamma);
                if (!BACKWARD)
                    cls_sum += v;
                else
                    gv[c >> 2][c & 3] = (float)((double)(v * a.cls_w * m) / total_fg) * gscale;
                continue;
            }
            const float e = expf(-fabsf(x));
            const float p = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            const float sp = fmaxf(x, 0.f) + log1pf(e);
            const float pg = a.gamma == 2.f ? p * p : powf(p, a.gamma);
            if (!BACKWARD) {
                const float bce = sp - x * t;
                cls_sum += t > 0.f ? t * bce : a.alpha * pg * bce;
            } else {
                const float g = t > 0.f ? t * (p - t) : a.alpha * pg * (a.gamma * (1.f - p) * sp + p);
                gv[c >> 2][c & 3] = (float)((double)(g * a.cls_w * m) / total_fg) * gscale;
            }
        }
        if (BACKWARD && row32) {
#pragma unroll
            for (int q = 0; q < 8; ++q) *(f32x4*)(a.d_logits + i * 32 + q * 4) = gv[q];
        }
        for (int c = row32 ? a.n_cls : 0; c < a.n_cls; ++c) {  // (other row lengths: the scalar loop)
            const float x = a.logits[i * a.ld_logits + c];
            const float t = (label == c) ? aff : 0.f;
            if (!BACKWARD && a.soft) a.soft[(b * a.n_cls + c) * hw + pix] = t;
            if (CLS >= 0) {
                const float v = cls_term<(CLS < 0 ? 0 : CLS), BACKWARD>(x, t, a.alpha, a.gamma);
                if (!BACKWARD)
                    cls_sum += v;
                else
                    a.d_logits[i * a.ld_logits + c] = (float)((double)(v * a.cls_w * m) / total_fg) * gscale;
                continue;
            }
            // one exponential per class serves the sigmoid and the softplus; p^gamma is a product for the recipe's gamma = 2
            // (the transcendental functions, not the 34 floats per pixel, are what this kernel's time goes to)
            const float e = expf(-fabsf(x));
            const float p = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            const float sp = fmaxf(x, 0.f) + log1pf(e);
            const float pg = a.gamma == 2.f ? p * p : powf(p, a.gamma);
            if (!BACKWARD) {
                const float bce = sp - x * t;  // BCE-with-logits
                const float l = t > 0.f ? t * bce : a.alpha * pg * bce;
                cls_sum += l;
            } else {
                float g;
                if (t > 0.f)
                    g = t * (p - t);
                else
                    g = a.alpha * pg * (a.gamma * (1.f - p) * sp + p);
                a.d_logits[i * a.ld_logits + c] = (float)((double)(g * a.cls_w * m) / total_fg) * gscale;
            }
        }
        // ---- regression: L1 (or reg_term of the configured kind) with the per-object normaliser in fp64 ----
        const bool reg_on = label < a.n_cls;
        const double norm = 1.0 / ((double)a.ppo[i] + (double)a.smoothing);
        if (!BACKWARD) {
            const double v = (double)(cls_sum * a.cls_w * m);
            acc[0] += v;
            if (fg) acc[1] += v;
            if (bg) acc[2] += v;
            if (fg) acc[3] += 1.0;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (reg_on) {
                    const float l = CLS >= 0 ? reg_term<false>(reg_kind, reg_param, r[j] - tg[j]) : fabsf(r[j] - tg[j]);
                    acc[4 + j] += (double)(l * a.reg_w) * norm * (double)m * (double)a.coding[j] / 8.0;
                }
        } else {
            float dr[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = r[j] - tg[j];
                const float sgn = CLS >= 0 ? reg_term<true>(reg_kind, reg_param, d) : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
                const double g = reg_on ? (double)(sgn * a.reg_w) * norm * (double)m * (double)a.coding[j] / 8.0 / total_obj : 0.0;
                dr[j] = (float)g * gscale;
            }
            *(f32x4*)(a.d_reg + i * a.ld_reg) = f32x4{dr[0], dr[1], dr[2], dr[3]};
            *(f32x4*)(a.d_reg + i * a.ld_reg + 4) = f32x4{dr[4], dr[5], dr[6], dr[7]};
        }
    }
    if (!BACKWARD) {
        // waves -> workgroup through LDS, then ONE fp64 atomic per workgroup and quantity (one per WAVE was 98 k atomics on
        // twelve addresses: the forward pass spent most of its time queueing at them)
        __shared__ double red[4][12];
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const double s = wave_sum_d(acc[j]);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s;
        }
        __syncthreads();
        if (threadIdx.x < 12) {
            const double s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
            if (s != 0.0) atomicAdd(&a.sums[threadIdx.x], s);
        }
    }
}

template <bool BACKWARD>
__global__ __launch_bounds__(256) void loss_kernel(const LossArgs a) {
    const double total_fg = BACKWARD ? a.sums[13] : 1.0;
    const double total_obj = BACKWARD ? a.sums[12] : 1.0;
    const float gscale = BACKWARD ? a.grad_scale * (float)a.sums[15] : 1.f;  // host factor x device factor (sums[15]: 1 unless the caller wrote the incoming gradient there)
    loss_tile<BACKWARD>(a, blockIdx.x, gridDim.x, total_fg, total_obj, gscale);
}

// ---- several (level, task) entries in ONE launch: the table travels by value as the kernel argument (<= 16 entries, ~2.3 KB: nothing
// to copy to the device and nothing to keep alive); a workgroup finds its entry by the prefix sums of the entries' workgroup counts ----
struct LossTable {
    int n;
    int block_begin[RV_ML_MAX_ENTRIES + 1];
    rvLossEntry e[RV_ML_MAX_ENTRIES];
    rvLossParams p;
    double* sums;  // (n + 1) rows of RV_LOSS_SUMS_LEN
    float grad_scale;
};

template <bool BACKWARD>
__global__ __launch_bounds__(256) void loss_table_kernel(const LossTable t) {
    int k = 0;
    while (k + 1 < t.n && (int)blockIdx.x >= t.block_begin[k + 1]) ++k;  // (wave-uniform: scalar loads)
    const rvLossEntry& e = t.e[k];
    LossArgs a;
    a.logits = e.logits;
    a.reg = e.regressands;
    a.cart = e.cart;
    a.mask = e.mask;
    a.labels = e.labels;
    a.panoptics = e.panoptics;
    a.reg_targets = e.reg_targets;
    a.ppo = e.points_per_obj;
    a.num_objects = e.num_objects;
    a.B = e.B;
    a.n_cls = e.n_cls;
    a.H = e.H;
    a.W = e.W;
    a.ld_logits = e.ld_logits;
    a.ld_reg = e.ld_reg;
#pragma unroll
    for (int j = 0; j < 8; ++j) a.coding[j] = t.p.coding_weights[j];
    a.cls_w = t.p.cls_weight;
    a.reg_w = t.p.reg_weight;
    a.smoothing = t.p.smoothing;
    a.sigma = t.p.sigma;
    a.alpha = t.p.alpha;
    a.gamma = t.p.gamma;
    a.az_inv = t.p.azimuth_invariant;
    a.sums = t.sums + (int64_t)k * RV_LOSS_SUMS_LEN;
    a.soft = e.soft_targets;
    a.fg = e.foreground;
    a.d_logits = e.d_logits;
    a.d_reg = e.d_regressands;
    a.grad_scale = t.grad_scale;
    // every level is normalised by the two GLOBAL numbers phase two left in its row; the incoming gradient sits in the totals row
    const double total_fg = BACKWARD ? a.sums[13] : 1.0;
    const double total_obj = BACKWARD ? a.sums[12] : 1.0;
    const float gscale = BACKWARD ? t.grad_scale * (float)t.sums[(int64_t)t.n * RV_LOSS_SUMS_LEN + 15] : 1.f;
    loss_tile<BACKWARD>(a, (int)blockIdx.x - t.block_begin[k], t.block_begin[k + 1] - t.block_begin[k], total_fg, total_obj, gscale);
}

// the LossArgs of entry k of the table, as loss_table_kernel fills them (that kernel keeps its own text: its machine code is unchanged)
__device__ __forceinline__ LossArgs table_args(const LossTable& t, int k) {
    const rvLossEntry& e = t.e[k];
    LossArgs a;
    a.logits = e.logits;
    a.reg = e.regressands;
    a.cart = e.cart;
    a.mask = e.mask;
    a.labels = e.labels;
    a.panoptics = e.panoptics;
    a.reg_targets = e.reg_targets;
    a.ppo = e.points_per_obj;
    a.num_objects = e.num_objects;
    a.B = e.B;
    a.n_cls = e.n_cls;
    a.H = e.H;
    a.W = e.W;
    a.ld_logits = e.ld_logits;
    a.ld_reg = e.ld_reg;
#pragma unroll
    for (int j = 0; j < 8; ++j) a.coding[j] = t.p.coding_weights[j];
    a.cls_w = t.p.cls_weight;
    a.reg_w = t.p.reg_weight;
    a.smoothing = t.p.smoothing;
    a.sigma = t.p.sigma;
    a.alpha = t.p.alpha;
    a.gamma = t.p.gamma;
    a.az_inv = t.p.azimuth_invariant;
    a.sums = t.sums + (int64_t)k * RV_LOSS_SUMS_LEN;
    a.soft = e.soft_targets;
    a.fg = e.foreground;
    a.d_logits = e.d_logits;
    a.d_reg = e.d_regressands;
    a.grad_scale = t.grad_scale;
    return a;
}

// the same with every entry's affinity read from its map (rv_soft_assign): the maps travel as a second by-value argument
struct AffMaps {
    const float* map[RV_ML_MAX_ENTRIES];
};

template <bool BACKWARD>
__global__ __launch_bounds__(256) void loss_table_aff_kernel(const LossTable t, const AffMaps maps) {
    int k = 0;
    while (k + 1 < t.n && (int)blockIdx.x >= t.block_begin[k + 1]) ++k;
    const LossArgs a = table_args(t, k);
    const double total_fg = BACKWARD ? a.sums[13] : 1.0;
    const double total_obj = BACKWARD ? a.sums[12] : 1.0;
    const float gscale = BACKWARD ? t.grad_scale * (float)t.sums[(int64_t)t.n * RV_LOSS_SUMS_LEN + 15] : 1.f;
    loss_tile<BACKWARD, true>(a, (int)blockIdx.x - t.block_begin[k], t.block_begin[k + 1] - t.block_begin[k], total_fg, total_obj, gscale, maps.map[k]);
}

// the table pair with loss kinds (rv_detection_loss_table_*): one instantiation per classification kind, the regression kind a uniform
// run-time switch; AFF_MAP as above.  The default recipe never launches these.
template <bool BACKWARD, bool AFF_MAP, int CLS>
__global__ __launch_bounds__(256) void loss_table_kinds_kernel(const LossTable t, const AffMaps maps, const int reg_kind, const float reg_param) {
    int k = 0;
    while (k + 1 < t.n && (int)blockIdx.x >= t.block_begin[k + 1]) ++k;
    const LossArgs a = table_args(t, k);
    const double total_fg = BACKWARD ? a.sums[13] : 1.0;
    const double total_obj = BACKWARD ? a.sums[12] : 1.0;
    const float gscale = BACKWARD ? t.grad_scale * (float)t.sums[(int64_t)t.n * RV_LOSS_SUMS_LEN + 15] : 1.f;
    loss_tile<BACKWARD, AFF_MAP, CLS>(a, (int)blockIdx.x - t.block_begin[k], t.block_begin[k + 1] - t.block_begin[k], total_fg, total_obj, gscale,
                                      AFF_MAP ? maps.map[k] : nullptr, reg_kind, reg_param);
}

// phase two (reduce_multiscale_loss, detection_head.py:379-449): the global normalisers, every entry's scalars, and their sums over
// the entry list.  One wave; lane e owns entry e (n <= 16), the totals go through wave shuffles.
__global__ __launch_bounds__(64) void loss_table_finish_kernel(const LossTable t) {
    const int e = threadIdx.x;
    const bool on = e < t.n;
    double* s = t.sums + (int64_t)(on ? e : 0) * RV_LOSS_SUMS_LEN;
    const double n_fg = wave_sum_d(on ? s[3] : 0.0);
    const double n_obj = wave_sum_d(on ? (double)*t.e[on ? e : 0].num_objects : 0.0);
    const double obj = n_obj < 1.0 ? 1.0 : n_obj, fg = n_fg + (double)t.p.smoothing;
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0;
    if (on) {
        const double coord = (s[4] + s[5] + s[6]) / obj, dim = (s[7] + s[8] + s[9]) / obj, rot = (s[10] + s[11]) / obj;
        const double cls = s[0] / fg, reg = (((((((s[4] + s[5]) + s[6]) + s[7]) + s[8]) + s[9]) + s[10]) + s[11]) / obj;
        v[0] = cls + reg;
        v[1] = cls;
        v[2] = s[1] / fg;
        v[3] = s[2] / fg;
        v[4] = coord;
        v[5] = dim;
        v[6] = rot;
        v[7] = coord + dim + rot;
        s[12] = obj;
        s[13] = fg;
        s[14] = 0.0;
        s[15] = 1.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) s[16 + j] = v[j];
    }
    double* tot = t.sums + (int64_t)t.n * RV_LOSS_SUMS_LEN;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double w = wave_sum_d(v[j]);
        if (e == 0) tot[16 + j] = w;
    }
    if (e == 0) {
        for (int j = 0; j < 12; ++j) tot[j] = 0.0;
        tot[12] = (double)t.n * obj;  // (the reference sums its collated list: n_entries x the value)
        tot[13] = (double)t.n * fg;
        tot[14] = 0.0;
        tot[15] = 1.0;
    }
}

__global__ void loss_finish_kernel(double* sums, const int32_t* num_objects, float smoothing) {
    const double n = (double)*num_objects;
    const double obj = n < 1.0 ? 1.0 : n, fg = sums[3] + (double)smoothing;
    sums[12] = obj;
    sums[13] = fg;
    sums[15] = 1.0;  // device-side factor of the backward pass (the caller copies the incoming gradient of the loss here: no host round trip)
    // the scalars detection_head.py:379-449 reports, formed here instead of by a dozen one-element launches on the host side
    const double coord = (sums[4] + sums[5] + sums[6]) / obj, dim = (sums[7] + sums[8] + sums[9]) / obj, rot = (sums[10] + sums[11]) / obj;
    const double cls = sums[0] / fg, reg = (((((((sums[4] + sums[5]) + sums[6]) + sums[7]) + sums[8]) + sums[9]) + sums[10]) + sums[11]) / obj;
    sums[16] = cls + reg;  // loss
    sums[17] = cls;
    sums[18] = sums[1] / fg;
    sums[19] = sums[2] / fg;
    sums[20] = coord;
    sums[21] = dim;
    sums[22] = rot;
    sums[23] = coord + dim + rot;
}

int fill(LossArgs* a, const float* logits, int32_t ld_logits, const float* reg, int32_t ld_reg, const float* cart,
         const uint8_t* mask, const int64_t* labels, const int64_t* panoptics, const float* reg_targets,
         const int64_t* ppo, const int32_t* num_objects, int32_t B, int32_t n_cls, int32_t H, int32_t W,
         const float* host_coding_weights, float cls_w, float reg_w, float smoothing, float sigma, float alpha, float gamma,
         int32_t az_inv, double* sums) {
    RV_REQUIRE(logits && reg && cart && mask && labels && panoptics && reg_targets && ppo && num_objects && sums && host_coding_weights,
               "rv_detection_loss: null argument");
    RV_REQUIRE(ld_logits >= n_cls && ld_reg >= 8 && ld_reg % 4 == 0, "rv_detection_loss: bad strides (rows of regressands must be 16-byte aligned)");
    memset(a, 0, sizeof(*a));
    a->logits = logits;
    a->reg = reg;
    a->cart = cart;
    a->mask = mask;
    a->labels = labels;
    a->panoptics = panoptics;
    a->reg_targets = reg_targets;
    a->ppo = ppo;
    a->num_objects = num_objects;
    a->B = B;
    a->n_cls = n_cls;
    a->H = H;
    a->W = W;
    a->ld_logits = ld_logits;
    a->ld_reg = ld_reg;
    for (int j = 0; j < 8; ++j) a->coding[j] = host_coding_weights[j];
    a->cls_w = cls_w;
    a->reg_w = reg_w;
    a->smoothing = smoothing;
    a->sigma = sigma;
    a->alpha = alpha;
    a->gamma = gamma;
    a->az_inv = az_inv;
    a->sums = sums;
    a->grad_scale = 1.f;
    return 0;
}

int grid_for(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

}  // namespace

extern "C" int rv_detection_loss_forward(const float* logits, int32_t ld_logits, const float* regressands, int32_t ld_reg,
                                         const float* cart, const uint8_t* mask, const int64_t* labels,
                                         const int64_t* panoptics, const float* reg_targets, const int64_t* points_per_obj,
                                         const int32_t* num_objects, int32_t B, int32_t n_cls, int32_t H, int32_t W,
                                         const float* host_coding_weights, float cls_weight, float reg_weight,
                                         float smoothing, float sigma, float alpha, float gamma, int32_t azimuth_invariant,
                                         double* sums, float* soft_targets, float* foreground, rvStream stream) {
    LossArgs a;
    if (fill(&a, logits, ld_logits, regressands, ld_reg, cart, mask, labels, panoptics, reg_targets, points_per_obj,
             num_objects, B, n_cls, H, W, host_coding_weights, cls_weight, reg_weight, smoothing, sigma, alpha, gamma,
             azimuth_invariant, sums))
        return 1;
    a.soft = soft_targets;
    a.fg = foreground;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(sums, 0, RV_LOSS_SUMS_LEN * sizeof(double), st);
    if (e != hipSuccess) RV_FAIL("rv_detection_loss_forward: %s", hipGetErrorString(e));
    const int fwd_grid = grid_for((int64_t)B * H * W) < 512 ? grid_for((int64_t)B * H * W) : 512;  // (grid-stride: fewer, longer workgroups -> fewer atomics)
    hipLaunchKernelGGL(loss_kernel<false>, dim3(fwd_grid), dim3(256), 0, st, a);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(1), 0, st, sums, num_objects, smoothing);
    RV_CHECK_LAUNCH("loss forward kernels");
    return 0;
}

extern "C" int rv_detection_loss_backward(const float* logits, int32_t ld_logits, const float* regressands, int32_t ld_reg,
                                          const float* cart, const uint8_t* mask, const int64_t* labels,
                                          const int64_t* panoptics, const float* reg_targets, const int64_t* points_per_obj,
                                          const int32_t* num_objects, int32_t B, int32_t n_cls, int32_t H, int32_t W,
                                          const float* host_coding_weights, float cls_weight, float reg_weight,
                                          float smoothing, float sigma, float alpha, float gamma, int32_t azimuth_invariant,
                                          const double* sums, float grad_scale, float* d_logits, float* d_regressands,
                                          rvStream stream) {
    LossArgs a;
    if (fill(&a, logits, ld_logits, regressands, ld_reg, cart, mask, labels, panoptics, reg_targets, points_per_obj,
             num_objects, B, n_cls, H, W, host_coding_weights, cls_weight, reg_weight, smoothing, sigma, alpha, gamma,
             azimuth_invariant, (double*)sums))
        return 1;
    RV_REQUIRE(d_logits && d_regressands, "rv_detection_loss_backward: null gradient buffers");
    a.d_logits = d_logits;
    a.d_reg = d_regressands;
    a.grad_scale = grad_scale;
    hipLaunchKernelGGL(loss_kernel<true>, dim3(grid_for((int64_t)B * H * W)), dim3(256), 0, (hipStream_t)stream, a);
    RV_CHECK_LAUNCH("loss backward kernel");
    return 0;
}

extern "C" int32_t rv_detection_loss_sums_len(void) { return RV_LOSS_SUMS_LEN; }

namespace {

int fill_table(LossTable* t, const rvLossEntry* entries, int32_t n, const rvLossParams* p, double* sums, bool backward) {
    RV_REQUIRE(entries && p && sums, "rv_detection_loss_multilevel: null argument");
    RV_REQUIRE(n >= 1 && n <= RV_ML_MAX_ENTRIES, "rv_detection_loss_multilevel: %d entries (1 .. %d)", n, RV_ML_MAX_ENTRIES);
    memset(t, 0, sizeof(*t));
    t->n = n;
    t->p = *p;
    t->sums = sums;
    t->grad_scale = 1.f;
    for (int k = 0; k < n; ++k) {
        const rvLossEntry& e = entries[k];
        RV_REQUIRE(e.logits && e.regressands && e.cart && e.mask && e.labels && e.panoptics && e.reg_targets && e.points_per_obj && e.num_objects,
                   "rv_detection_loss_multilevel: null tensor in entry %d", k);
        RV_REQUIRE(e.B > 0 && e.H > 0 && e.W > 0 && e.n_cls > 0, "rv_detection_loss_multilevel: bad shape in entry %d", k);
        RV_REQUIRE(e.ld_logits >= e.n_cls && e.ld_reg >= 8 && e.ld_reg % 4 == 0,
                   "rv_detection_loss_multilevel: bad strides in entry %d (rows of regressands must be 16-byte aligned)", k);
        RV_REQUIRE(!backward || (e.d_logits && e.d_regressands), "rv_detection_loss_multilevel_backward: null gradient buffers in entry %d", k);
        t->e[k] = e;
        const int64_t work = (int64_t)e.B * e.H * e.W;
        // the one-level entry points' grids, entry by entry (forward: grid-stride with at most 512 workgroups -> fewer atomics)
        const int blocks = backward ? grid_for(work) : (grid_for(work) < 512 ? grid_for(work) : 512);
        t->block_begin[k + 1] = t->block_begin[k] + blocks;
    }
    return 0;
}

}  // namespace

extern "C" int rv_detection_loss_multilevel_forward(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                                    double* sums, rvStream stream) {
    LossTable t;
    if (fill_table(&t, host_entries, n_entries, host_params, sums, false)) return 1;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)(n_entries + 1) * RV_LOSS_SUMS_LEN * sizeof(double), st);
    if (e != hipSuccess) RV_FAIL("rv_detection_loss_multilevel_forward: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(loss_table_kernel<false>, dim3(t.block_begin[n_entries]), dim3(256), 0, st, t);
    hipLaunchKernelGGL(loss_table_finish_kernel, dim3(1), dim3(64), 0, st, t);
    RV_CHECK_LAUNCH("multi-level loss forward kernels");
    return 0;
}

extern "C" int rv_detection_loss_multilevel_backward(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                                     const double* sums, float grad_scale, rvStream stream) {
    LossTable t;
    if (fill_table(&t, host_entries, n_entries, host_params, (double*)sums, true)) return 1;
    t.grad_scale = grad_scale;
    hipLaunchKernelGGL(loss_table_kernel<true>, dim3(t.block_begin[n_entries]), dim3(256), 0, (hipStream_t)stream, t);
    RV_CHECK_LAUNCH("multi-level loss backward kernel");
    return 0;
}

namespace {

int fill_maps(AffMaps* maps, const float* const* host_maps, int32_t n) {
    RV_REQUIRE(host_maps, "rv_detection_loss_multilevel_*_aff: null affinity maps");
    memset(maps, 0, sizeof(*maps));
    for (int k = 0; k < n; ++k) {
        RV_REQUIRE(host_maps[k], "rv_detection_loss_multilevel_*_aff: null affinity map of entry %d", k);
        maps->map[k] = host_maps[k];
    }
    return 0;
}

}  // namespace

extern "C" int rv_detection_loss_multilevel_forward_aff(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                                        const float* const* host_affinity_maps, double* sums, rvStream stream) {
    LossTable t;
    AffMaps maps;
    if (fill_table(&t, host_entries, n_entries, host_params, sums, false) || fill_maps(&maps, host_affinity_maps, n_entries)) return 1;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)(n_entries + 1) * RV_LOSS_SUMS_LEN * sizeof(double), st);
    if (e != hipSuccess) RV_FAIL("rv_detection_loss_multilevel_forward_aff: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(loss_table_aff_kernel<false>, dim3(t.block_begin[n_entries]), dim3(256), 0, st, t, maps);
    hipLaunchKernelGGL(loss_table_finish_kernel, dim3(1), dim3(64), 0, st, t);
    RV_CHECK_LAUNCH("multi-level loss forward kernels (affinity maps)");
    return 0;
}

extern "C" int rv_detection_loss_multilevel_backward_aff(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                                         const float* const* host_affinity_maps, const double* sums, float grad_scale,
                                                         rvStream stream) {
    LossTable t;
    AffMaps maps;
    if (fill_table(&t, host_entries, n_entries, host_params, (double*)sums, true) || fill_maps(&maps, host_affinity_maps, n_entries)) return 1;
    t.grad_scale = grad_scale;
    hipLaunchKernelGGL(loss_table_aff_kernel<true>, dim3(t.block_begin[n_entries]), dim3(256), 0, (hipStream_t)stream, t, maps);
    RV_CHECK_LAUNCH("multi-level loss backward kernel (affinity maps)");
    return 0;
}

namespace {

int check_kinds(const rvLossKinds* kinds) {
    RV_REQUIRE(kinds, "rv_detection_loss_table: null kinds");
    RV_REQUIRE(kinds->cls_kind >= RV_CLS_VARIFOCAL && kinds->cls_kind <= RV_CLS_PENALTY_REDUCED, "rv_detection_loss_table: unknown classification kind %d",
               kinds->cls_kind);
    RV_REQUIRE(kinds->reg_kind >= RV_REG_L1 && kinds->reg_kind <= RV_REG_MSE, "rv_detection_loss_table: unknown regression kind %d", kinds->reg_kind);
    if (kinds->reg_kind == RV_REG_SMOOTH_L1 || kinds->reg_kind == RV_REG_HUBER) {
        RV_REQUIRE(std::isfinite(kinds->reg_param), "rv_detection_loss_table: reg_param is not finite");
        RV_REQUIRE(kinds->reg_kind != RV_REG_SMOOTH_L1 || kinds->reg_param >= 0.f, "rv_detection_loss_table: SMOOTH_L1 needs beta >= 0, not %g",
                   (double)kinds->reg_param);
        RV_REQUIRE(kinds->reg_kind != RV_REG_HUBER || kinds->reg_param > 0.f, "rv_detection_loss_table: HUBER needs delta > 0, not %g", (double)kinds->reg_param);
    }
    return 0;
}

template <bool BACKWARD, bool AFF_MAP>
void launch_kinds(const LossTable& t, const AffMaps& maps, const rvLossKinds& k, hipStream_t st) {
    const dim3 grid(t.block_begin[t.n]), block(256);
    switch (k.cls_kind) {
        case RV_CLS_FOCAL:
            hipLaunchKernelGGL((loss_table_kinds_kernel<BACKWARD, AFF_MAP, RV_CLS_FOCAL>), grid, block, 0, st, t, maps, k.reg_kind, k.reg_param);
            break;
        case RV_CLS_PENALTY_REDUCED:
            hipLaunchKernelGGL((loss_table_kinds_kernel<BACKWARD, AFF_MAP, RV_CLS_PENALTY_REDUCED>), grid, block, 0, st, t, maps, k.reg_kind, k.reg_param);
            break;
        default:
            hipLaunchKernelGGL((loss_table_kinds_kernel<BACKWARD, AFF_MAP, RV_CLS_VARIFOCAL>), grid, block, 0, st, t, maps, k.reg_kind, k.reg_param);
    }
}

}  // namespace

extern "C" int rv_detection_loss_table_forward(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                               const rvLossKinds* host_kinds, const float* const* host_affinity_maps, double* sums, rvStream stream) {
    LossTable t;
    AffMaps maps;
    memset(&maps, 0, sizeof(maps));
    if (check_kinds(host_kinds) || fill_table(&t, host_entries, n_entries, host_params, sums, false)) return 1;
    if (host_affinity_maps && fill_maps(&maps, host_affinity_maps, n_entries)) return 1;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)(n_entries + 1) * RV_LOSS_SUMS_LEN * sizeof(double), st);
    if (e != hipSuccess) RV_FAIL("rv_detection_loss_table_forward: %s", hipGetErrorString(e));
    if (host_affinity_maps)
        launch_kinds<false, true>(t, maps, *host_kinds, st);
    else
        launch_kinds<false, false>(t, maps, *host_kinds, st);
    hipLaunchKernelGGL(loss_table_finish_kernel, dim3(1), dim3(64), 0, st, t);
    RV_CHECK_LAUNCH("loss table forward kernels");
    return 0;
}

extern "C" int rv_detection_loss_table_backward(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                                const rvLossKinds* host_kinds, const float* const* host_affinity_maps, const double* sums,
                                                float grad_scale, rvStream stream) {
    LossTable t;
    AffMaps maps;
    memset(&maps, 0, sizeof(maps));
    if (check_kinds(host_kinds) || fill_table(&t, host_entries, n_entries, host_params, (double*)sums, true)) return 1;
    if (host_affinity_maps && fill_maps(&maps, host_affinity_maps, n_entries)) return 1;
    t.grad_scale = grad_scale;
    if (host_affinity_maps)
        launch_kinds<true, true>(t, maps, *host_kinds, (hipStream_t)stream);
    else
        launch_kinds<true, false>(t, maps, *host_kinds, (hipStream_t)stream);
    RV_CHECK_LAUNCH("loss table backward kernel");
    return 0;
}
