// ewpass.h -- which kernel form each bandwidth-bound BatchNorm / element-wise pass launches, decided in ONE place: the entry
// points of misc.hip and bnbwd.hip launch from these plans and rv_ew_pass_info (bnbwd.hip) reports them, so a test that asserts the
// form of its own shape and the launch it then makes cannot disagree.  Host code only.
#pragma once
#include <algorithm>

#include "common.h"

struct RvEwPlan {
    int form;         // RV_EW_FORM_*
    int nontemporal;  // 1: streaming (non-temporal) loads and stores
    int grid;         // workgroups of the (last) launch
    int index;        // template argument of the kernel instantiation (see rv_ew_pass_info in include/rv3d.h)
};

// the lean (quad layout, <= 96 VGPRs) forms of the four BatchNorm-backward passes are what runs; the octet forms take tensors whose byte
// offsets do not fit 32 bits (A/B of the two and of a one-workgroup-per-CU launch: profiles/r04_ab_notes.md)
constexpr int rv_bnb_lean() { return 2; }

// tensors that exceed the 256 MB Infinity Cache anyway: streaming loads / stores (profiles/r02_hbm_kernels.md)
static inline bool rv_ew_beyond_cache(int64_t pixels, int c) { return pixels * c * 2 >= ((int64_t)256 << 20); }

// the lean forms keep 32-bit byte offsets from the tensor bases and one channel quad per thread (at most 256 quads)
static inline bool rv_bnb_takes_lean(int64_t pixels, int c, int64_t ld_max) {
    return rv_bnb_lean() && c <= 1024 && pixels * ld_max * 2 < ((int64_t)1 << 32);
}

// grid-stride comb over `work` items, 256 per workgroup pass
static inline int rv_ew_comb_grid(int64_t work) {
    int64_t b = (work + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

// one contiguous pixel range per workgroup, `lanes_px` pixels per pass
static inline int rv_ew_range_grid(int64_t pixels, int lanes_px) {
    int64_t blocks = (pixels + lanes_px - 1) / lanes_px;
    return (int)(blocks > 4096 ? 4096 : blocks);
}

// rv_ew_combine.  (measured, profiles/r02_hbm_kernels.md: the row-range kernel wins on tensors beyond the Infinity Cache, 4.9-5.2 vs
// 4.7-4.8 TB/s; on small ones its per-thread constant prologue costs more than the comb's address arithmetic, 2.9 vs 6.2 TB/s)
static inline RvEwPlan rv_plan_ew_combine(int64_t pixels, int c, bool has_b) {
    const int c8 = c / 8;
    if (c8 <= 256 && rv_ew_beyond_cache(pixels, c)) return {RV_EW_FORM_ROWS, 1, rv_ew_range_grid(pixels, 256 / c8), has_b ? 1 : 0};
    return {RV_EW_FORM_COMB, 0, rv_ew_comb_grid(pixels * c8), 0};
}

static inline RvEwPlan rv_plan_ew_mask_grad(int64_t pixels, int c) { return {RV_EW_FORM_COMB, 0, rv_ew_comb_grid(pixels * (c / 8)), 0}; }

static inline int64_t rv_max_ld(int64_t a, int64_t b, int64_t c = 0, int64_t d = 0, int64_t e = 0) {
    return std::max(std::max(std::max(a, b), std::max(c, d)), e);
}

// rv_bn_bwd_reduce (index = OUT of the lean kernel); the guard takes every row pitch as passed, ld_out of an absent `out` included
static inline RvEwPlan rv_plan_bnb_reduce(int64_t pixels, int c, int ld_dout, int ld_out, int ld_y, bool has_out) {
    const int grid = rv_bn_bwd_rows(pixels);
    if (rv_bnb_takes_lean(pixels, c, rv_max_ld(ld_dout, ld_y, ld_out))) return {RV_EW_FORM_LEAN, 0, grid, has_out ? 1 : 0};
    return {RV_EW_FORM_OCTET, 0, grid, 0};
}

static inline RvEwPlan rv_plan_bnb_reduce_pair(int64_t pixels, int c, int ld_dout, int ld_out, int ld_ya, int ld_yb) {
    const int grid = rv_bn_bwd_rows(pixels);
    if (rv_bnb_takes_lean(pixels, c, rv_max_ld(ld_dout, ld_out, ld_ya, ld_yb))) return {RV_EW_FORM_LEAN, 0, grid, 0};
    return {RV_EW_FORM_OCTET, 0, grid, 0};
}

// rv_bn_bwd_apply.  Lean form: index = F of bn_bwd_apply_lean_kernel<F> (bit 0 streaming, bit 1 ReLU mask tensor, bit 2
// residual-gradient output, bit 3 accumulated onto what is there); octet form: index = MODE.
static inline RvEwPlan rv_plan_bnb_apply(int64_t pixels, int c, int ld_dout, int ld_out, int ld_y, int ld_dy, int ld_dres, bool has_out,
                                         bool has_dres, int flags) {
    const int nt = rv_ew_beyond_cache(pixels, c) ? 1 : 0;
    if (rv_bnb_takes_lean(pixels, c, rv_max_ld(ld_dout, ld_y, ld_out, ld_dy, ld_dres)))
        return {RV_EW_FORM_LEAN, nt, rv_ew_range_grid(pixels, 256 / (c / 4)),
                nt | (has_out ? 2 : 0) | (has_dres ? 4 : 0) | (has_dres && (flags & RV_BNB_RES_ACCUM) ? 8 : 0)};
    return {RV_EW_FORM_OCTET, nt, rv_ew_range_grid(pixels, 256 / (c / 8)), nt};
}

// rv_bn_bwd_apply_pair: octet form only; index = MODE
static inline RvEwPlan rv_plan_bnb_apply_pair(int64_t pixels, int c) {
    const int nt = rv_ew_beyond_cache(pixels, c) ? 1 : 0;
    return {RV_EW_FORM_OCTET, nt, rv_ew_range_grid(pixels, 256 / (c / 8)), nt};
}

// rv_bn_finalize / rv_bn_bwd_finalize.  Few partial rows: one launch reduces and finalises; many (4096 rows behind a 512-channel
// tapconv4 launch): the 64-group column reduction spreads them over the chip first (29 us vs 14 us measured for the single launch).
static inline RvEwPlan rv_plan_bn_finalize(int rows, int c) {
    if (rows <= 2048) return {RV_EW_FORM_FUSED_FINALIZE, 0, rv_ceil_div(c, 16), 0};
    return {RV_EW_FORM_TWO_STAGE, 0, rv_ceil_div(c, 64), 0};
}
