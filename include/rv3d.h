/*
 * rv3d.h -- C ABI of librv3d_hip.so: the MI355X (gfx950) implementation of the range-view
 * detector's data-parallel hot path.
 *
 * Drop-in boundary.  The reference (benjaminrwilson/range-view-3d-detection, `torchbox3d`)
 * is pure Python; the native code it reaches on this path is (a) ATen/cuDNN kernels behind
 * torch.nn modules and (b) ONE explicit op-level FFI, `weighted_nms_ext.wnms_gpu`
 * (src/torchbox3d/math/ops/nms.py:161-170).  Every entry point below names the reference
 * interface it replaces (paths relative to the reference root, `src/torchbox3d/` elided
 * where unambiguous).  The Python host (`range_view_3d_detection_amd`) binds these symbols
 * with ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - Plain C: pointers + sizes.  All pointers are DEVICE pointers unless named `host_*`.
 *   - The caller (PyTorch's caching allocator in practice) owns every buffer; the library
 *     never allocates, frees or retains a pointer beyond the call (workspaces are passed in).
 *   - Every launch is enqueued on `stream` (a hipStream_t passed as void*); calls are
 *     asynchronous unless documented otherwise (only rv_wnms returns a host count).
 *   - Return value: 0 on success, non-zero on error; rv_last_error() returns a thread-local
 *     description.  Shapes are validated on the host before any launch.
 *   - Activations are NHWC ("pixel-major"): pixel (n,h,w) of a tensor with channel stride
 *     `ld` starts at element ((n*H + h)*W + w)*ld.  Activations / activation gradients are
 *     bf16 (uint16 storage); statistics, parameters, parameter gradients and the final
 *     head outputs are fp32.  Stored channel counts are multiples of 32, zero padded.
 *   - No global mutable state except a read-only device-property cache; safe to use from
 *     one process per GPU (the reference's Lightning-DDP process model).
 */
#ifndef RV3D_H_
#define RV3D_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rvStream; /* hipStream_t */

int rv_version(void);
const char* rv_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Tap geometry of one convolution-like layer.
 *
 * A layer owns a torch-layout weight T[cu][cv][kh][kw] and relates a "coarse" tensor U
 * (N,H,Wu,cu) to a "fine" tensor V (N,H,Wv,cv) through
 *       (hu, wu, ky, kx)  <->  (hv, wv) = (hu + ky - pad_h, wu*stride_w + kx - pad_w).
 *   nn.Conv2d (via Conv2dSame, nn/modules/conv.py:25-80; torchvision Conv2dNormActivation in
 *   nn/heads/dense_head.py:32-57, nn/stems/__init__.py:41-62):
 *       forward  y = GATHER(x)   (U = y, V = x, T = weight[co][ci][kh][kw])
 *       d/dx     dx = SCATTER(dy)
 *   nn.ConvTranspose2d (nn/blocks/__init__.py:149-156):
 *       forward  y = SCATTER(x)  (U = x, V = y, T = weight[ci][co][kh][kw])
 *       d/dx     dx = GATHER(dy)
 *   weight gradient (both): dT[cu][cv][ky][kx] = sum_{n,hu,wu} U[n,hu,wu,cu] * V[n,hv,wv,cv].
 * Vertical stride is 1 everywhere in this model (nn/backbones/dla.py:37-108).
 * ------------------------------------------------------------------------------------- */
typedef struct {
    int32_t kh, kw;       /* kernel extent */
    int32_t stride_w;     /* 1, 2 or 4 */
    int32_t pad_h, pad_w; /* zero padding (top/left); Conv2dSame: (k-1)/2 */
    int32_t cu, cv;       /* logical channel counts of U and V */
} rvTapGeom;

/* padded channel count used for every stored tensor / packed weight: round up to 32 */
int32_t rv_pad_channels(int32_t c);

/* Bytes of the packed bf16 weight images (gather / scatter form) for a geometry. */
int64_t rv_packed_weight_bytes(const rvTapGeom* g);

/* T (fp32, torch layout [cu][cv][kh][kw]) -> bf16 tap-major images with zero channel padding:
 *   gather_w  [tap = ky*kw+kx][cu_pad][cv_pad]               (K dim = cv contiguous)
 *   scatter_w [phase][tap-in-phase][cv_pad][cu_pad]          (K dim = cu contiguous)
 * Either output may be NULL.  Replaces nothing in the reference (cuDNN re-lays weights
 * internally); it is what keeps `state_dict()` in the reference's OIHW layout. */
int rv_pack_weight(const rvTapGeom* g, const float* T, void* gather_w, void* scatter_w, rvStream stream);

/* All layers of a model in ONE launch (every packed image is stale after an optimiser step; ~160 layers on the rv-* models).
 * The caller keeps a table of 2 entries per layer (gather image, scatter image; rv_pack_batch_entry_bytes() each): filled on
 * the HOST by rv_pack_batch_fill (pointers are device pointers), copied to the device once, and re-used every step for as
 * long as the parameter and image buffers stay where they are. */
int64_t rv_pack_batch_entry_bytes(void);
int rv_pack_batch_fill(const rvTapGeom* g, const float* T, void* gather_w, void* scatter_w, void* host_entries);
int rv_pack_batch(const void* dev_table, int32_t n_entries, rvStream stream);

/* FOLDED form of a stride-s layer (stride_w 2 or 4): the s fine pixels of a coarse pixel are contiguous in NHWC, so the fine
 * tensor V (N,H,s*Wu,cv_pad) read as (N,H,Wu,s*cv_pad) turns U = GATHER_s(V) -- a strided Conv2d's forward, a
 * ConvTranspose2d's backward-data -- and the layer's weight gradient into STRIDE-1 operations with kw' <= 3 column taps over
 * s*cv_pad channels, which the LDS-DMA kernels take (the strided forms run on the generic kernel at a third of the rate; the
 * zero entries of the folded weight cost 1.3-1.5x the FLOPs).  rv_fold_geom gives the folded geometry (use it with
 * rv_tap_gather / rv_tap_wgrad, Wv = Wu, ld of V multiplied by s; requires ld(V) == cv_pad), rv_pack_weight_folded its packed
 * gather image (rv_packed_weight_bytes(gf) bytes), rv_unfold_weight_grad maps a folded weight gradient (torch layout
 * [cu][s*cv_pad][kh][kw']) back to dT[cu][cv][kh][kw]. */
int rv_fold_geom(const rvTapGeom* g, rvTapGeom* folded);
int rv_pack_weight_folded(const rvTapGeom* g, const float* T, void* gather_w_folded, rvStream stream);
int rv_pack_batch_fill_folded(const rvTapGeom* g, const float* T, void* gather_w_folded, void* host_entry);
int rv_unfold_weight_grad(const rvTapGeom* g, const float* dT_folded, float* dT, int32_t accumulate, rvStream stream);

/* fp32 packed weight gradient [kh*kw][cu_pad][cv_pad] -> accumulate/store into torch layout
 * dT[cu][cv][kh][kw] (fp32).  accumulate != 0: dT += value. */
int rv_unpack_weight_grad(const rvTapGeom* g, const float* packed, float* dT, int32_t accumulate, rvStream stream);

/* flags for rv_tap_gather / rv_tap_scatter */
#define RV_IN_AFFINE 1   /* operand = in_scale[c]*x + in_shift[c] (folded BatchNorm) */
#define RV_IN_RELU 2     /* ... followed by ReLU; padding positions stay exactly 0 */
#define RV_OUT_F32 4     /* dst is fp32 (final head convs); default bf16 */
#define RV_OUT_BIAS 8    /* dst += bias[c] */
#define RV_OUT_STATS 16  /* write per-block partial sum / sum-of-squares of the fp32 result */
#define RV_OUT_ACCUM 32  /* dst += result (gradient fan-in); bf16 dst only */
#define RV_OUT_RELU 64   /* with RV_OUT_BIAS: dst = max(result + bias[c], 0) -- inference: an eval-mode BatchNorm folded into the
                          * weights (w * gamma / sqrt(var + eps)) and the bias (beta - mean * scale), ReLU in the epilogue, so that
                          * conv -> BatchNorm -> ReLU is ONE launch and one write (cuDNN conv + batch_norm + relu_ in the reference) */
#define RV_OUT_RES_RELU 256 /* rv_tap_residual only: ReLU AFTER the residual has been added (RV_OUT_RELU: before) */
#define RV_WGRAD_TORCH_LAYOUT 128 /* rv_tap_wgrad only: dT_packed receives the torch layout dT[cu][cv][kh][kw] (cu*cv*kh*kw fp32,
                                  * no padding) straight from the split-K reduction -- no rv_unpack_weight_grad pass */
/* Kernel-selection hints, also in rvTapShape.flags: speed heuristics only, never results.  PER CALL -- the library keeps no
 * mutable state; the parity tests use them so that crops the CPU oracle can afford run the kernels of the
 * full-size sweeps, and to pin a kernel generation. */
#define RV_SEL_SMALL_GRIDS (1 << 20)  /* the LDS-DMA tap-convs of generations 4 and 5 also take layers with fewer tiles than CUs */
#define RV_SEL_SMALL_GRIDS6 (1 << 21) /* ... and generation 6 */
#define RV_SEL_NO_GEN6 (1 << 22)      /* do not select generation 6 */
#define RV_SEL_NO_GEN5 (1 << 23)      /* do not select generations 5 and 6 (multi-tap layers stay on generation 4) */
#define RV_SEL_NO_POINTWISE (1 << 24) /* 1x1 C -> C layers stay on the tiled kernels (generation 7 = the pointwise streaming GEMM, round 6) */
#define RV_SEL_NO_POINTWISE_BWD (1 << 25) /* ... only its SCATTER-form (backward-data) launches stay on the tiled kernels (diagnostics: profiles/r06_ab_notes.md section 4) */
#define RV_SEL_MASK (63 << 20)

typedef struct {
    int32_t N, H, Wu, Wv; /* U is (N,H,Wu), V is (N,H,Wv) */
    int32_t ld_src, ld_dst; /* channel strides (elements) of the source / destination tensors */
    int32_t flags;
} rvTapShape;

/* Rows of the partial-statistics buffer ([rows][2][c_pad] fp32) a launch with RV_OUT_STATS
 * writes; `scatter` selects the SCATTER form.
 * The planning entry points (this one, rv_tap_launch_info, rv_tap_wgrad_info, rv_tap_wgrad_workspace_bytes, rv_tap_bnb_rows) size
 * persistent grids by the compute-unit count of the CURRENT device (hipGetDevice + one cached attribute query per device): they
 * launch nothing but they do initialise the HIP runtime -- call them after any fork and after GPU_MAX_HW_QUEUES is in the
 * environment; without a visible device they plan for 256 compute units. */
int32_t rv_tap_stats_rows(const rvTapGeom* g, const rvTapShape* s, int32_t scatter);
/* Launch plan the library picks for a tap op: info = {kernel generation, variant, grid.x, grid.y}:
 * generation 1 = tapconv_kernel<MT,NT> (variant = 16*MT + NT, block tile 32*MT pixels x 32*NT channels),
 * generation 2 = tapconv2_kernel<KS> (variant = KS, block tile 2 rows x 64 columns x 128 channels, 32*KS-channel
 * chunks), generations 4 / 5 / 6 = the LDS-DMA kernels (variant = channels per workgroup, grid.x = pixel tiles, grid.y = channel
 * tiles), generation 7 = the pointwise streaming GEMM (1x1 stride-1 C -> C layers, C = 256 / 128: variant = C, grid.x = persistent
 * workgroups).  Used by bench.py to label per-kernel timings. */
int rv_tap_launch_info(const rvTapGeom* g, const rvTapShape* s, int32_t scatter, int32_t* host_info);
/* Every partial-statistics buffer handed to rv_bn_finalize / rv_bn_bwd_finalize must have room
 * for this many extra rows after its `rows` partial rows (second-stage reduction scratch). */
#define RV_STATS_SCRATCH_ROWS 128

/* U = GATHER(V):  U[n,h,wu,cu] = sum_{ky,kx,cv} T[cu][cv][ky][kx] * f(V[n, h+ky-pad_h, wu*s+kx-pad_w, cv]).
 * Replaces nn.Conv2d forward (cuDNN/ATen conv2d; nn/modules/conv.py:80) including the
 * F.pad copy of Conv2dSame (:79), the preceding BatchNorm2d+ReLU when RV_IN_AFFINE|RV_IN_RELU
 * (nn/blocks/__init__.py:41-42), and ATen's conv_transpose2d backward-data. */
int rv_tap_gather(const rvTapGeom* g, const rvTapShape* s, const void* V, const float* in_scale,
                  const float* in_shift, const void* gather_w, const float* bias, void* U,
                  float* stats_partial, rvStream stream);

/* V = SCATTER(U): V[n,h,wv,cv] = sum over (ky,kx,wu) with wu*s+kx-pad_w == wv of
 *                 T[cu][cv][ky][kx] * f(U[n, h-ky+pad_h, wu, cu]).
 * Replaces nn.ConvTranspose2d forward (ATen conv_transpose2d; nn/blocks/__init__.py:176)
 * and cuDNN's conv2d backward-data. */
int rv_tap_scatter(const rvTapGeom* g, const rvTapShape* s, const void* U, const float* in_scale,
                   const float* in_shift, const void* scatter_w, const float* bias, void* V,
                   float* stats_partial, rvStream stream);

/* Inference: a tap op (scatter != 0: the SCATTER form) whose epilogue adds a residual tensor of the output's pixels,
 *   dst = [relu]( [relu]( op(src) + bias ) + res ),   s->flags: RV_OUT_BIAS, RV_OUT_RELU (inner), RV_OUT_RES_RELU (outer),
 * with the eval-mode BatchNorm folded into w / bias: the block outputs relu_(net(x) + proj(x)) of BasicBlock.forward
 * (nn/blocks/__init__.py:68-81) and x1 + relu(bn(convT(x2))) of AggregationBlock.forward (:165-182) leave the conv's own
 * launch -- no separate element-wise pass (ATen add + relu_ in the reference).  The result is the one the separate pass
 * produces, bit for bit: the conv result is rounded to the storage type before the residual is added, as a stored tensor
 * would have been.  res: bf16/fp16 [pixels of dst][ld_res]; plain operands only (no RV_IN_*, RV_OUT_STATS, RV_OUT_F32). */
int rv_tap_residual(const rvTapGeom* g, const rvTapShape* s, int32_t scatter, const void* src, const void* w, const float* bias,
                    const void* res, int32_t ld_res, void* dst, rvStream stream);

/* Backward-data launch that ALSO forms the BatchNorm-backward sums of the layer whose output gradient it writes
 * (conv -> BatchNorm(+ReLU) -> THIS conv: autograd's native_batch_norm_backward reduce over (dOut, y), fused into the
 * epilogue of conv2d backward-data).  dx = the gradient w.r.t. the (activated) BatchNorm output, written as by
 * rv_tap_gather / rv_tap_scatter (scatter != 0: the SCATTER form) without RV_OUT_ACCUM; from the bf16 values it stores,
 *   g = dx * [scale*y+shift > 0 if flags & RV_BNB_RELU_Z],   partial[row][0][c] = sum g,  partial[row][1][c] = sum g * (y-mean)*invstd
 * over the row's pixels -- the layout rv_bn_bwd_finalize takes (rv_bn_bwd_reduce then is not needed).
 * rv_tap_bnb_rows: partial rows such a launch writes; 0 = the kernel (g, s) selects has no such epilogue (generations 5 and 6
 * have it, for non-accumulating launches): use rv_tap_gather/scatter + rv_bn_bwd_reduce. */
typedef struct rvBnbEpilogue {
    const void* y;      /* bf16 NHWC pre-BatchNorm conv output of the destination layer, same pixels as dx */
    int32_t ld_y;       /* its channel stride (elements) */
    int32_t flags;      /* RV_BNB_RELU_Z */
    const float* scale; /* folded BatchNorm: gamma*invstd, beta - mean*scale (the ReLU mask) */
    const float* shift;
    const float* mean;
    const float* invstd;
    float* partial;     /* [rows + RV_STATS_SCRATCH_ROWS][2][c_pad] fp32 */
} rvBnbEpilogue;
int32_t rv_tap_bnb_rows(const rvTapGeom* g, const rvTapShape* s, int32_t scatter);
int rv_tap_data_grad_bnb(const rvTapGeom* g, const rvTapShape* s, int32_t scatter, const void* dout, const void* w, void* dx,
                         const rvBnbEpilogue* e, rvStream stream);

/* Weight gradient.  dT_packed[tap][cu_pad][cv_pad] (fp32) = sum_{n,h,wu} U * f(V) (shifted).
 * `workspace` holds split-K partial slabs; rv_tap_wgrad_workspace_bytes() sizes it.
 * V may carry the same folded BN+ReLU as in the forward (RV_IN_AFFINE|RV_IN_RELU in
 * s->flags applies to V when v_affine != 0, else to U).
 * Replaces cuDNN conv2d backward-weight / ATen conv_transpose2d backward-weight.
 * All three entry points plan alike and refuse what the launch refuses (a null g or s, kh*kw above 24 taps, Wv != Wu * stride_w, an
 * empty tensor): rv_tap_wgrad_workspace_bytes then returns -1, rv_tap_wgrad_info nonzero, both with rv_last_error() set. */
int64_t rv_tap_wgrad_workspace_bytes(const rvTapGeom* g, const rvTapShape* s);
/* host-side introspection (bench / tests): info[0] = kernel generation that rv_tap_wgrad will launch for (g, s)
 * (1 generic, 2 register-staged 3-tap groups, 3 LDS-DMA ring), info[1] = split-K factor, info[2] = workgroups */
int rv_tap_wgrad_info(const rvTapGeom* g, const rvTapShape* s, int32_t* host_info);
int rv_tap_wgrad(const rvTapGeom* g, const rvTapShape* s, const void* U, int32_t ld_u, const void* V, int32_t ld_v,
                 const float* in_scale, const float* in_shift, int32_t v_affine, float* dT_packed,
                 void* workspace, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * BatchNorm2d (nn.BatchNorm2d train/eval; nn/blocks/__init__.py:41,51,63,158; torchvision
 * Conv2dNormActivation norm layer).  eps / momentum are torch defaults passed by the host.
 * ------------------------------------------------------------------------------------- */
/* partial[rows][2][c] (sum, sum of squares) -> batch mean / biased var -> folded affine
 * scale = gamma*invstd, shift = beta - mean*scale; saves mean/invstd for backward and
 * updates running_mean / running_var (unbiased) in place when they are non-NULL. */
/* Column sums of `rows` partial rows ([rows][cols] fp32, accumulated in fp64) -> out[cols]; `partial` must have the
 * scratch rows of the convention above behind it.  SyncBN: totals written straight into the all-reduce buffer. */
int rv_reduce_rows(const float* partial, int32_t rows, int32_t cols, float* out, rvStream stream);
/* The same in the layout of one SyncBN collective: out[0 : cols] = the totals, out[cols] = `count` (this rank's element count,
 * summed by the all-reduce with the totals); out_copy (may be NULL) receives the LOCAL totals too -- in the backward pass
 * they are this rank's (dbeta, dgamma), which stay local (DDP averages parameter gradients).  One launch. */
int rv_reduce_rows_count(const float* partial, int32_t rows, int32_t cols, float count, float* out, float* out_copy, rvStream stream);
/* count < 0 (SyncBN, rows == 1): the element count is read from the device, partial[2*c] (fp32), where it travelled with
 * the all-reduced totals -- ranks may hold different numbers of pixels.  Same convention in rv_bn_bwd_finalize. */
int rv_bn_finalize(const float* partial, int32_t rows, int32_t c, int64_t count, const float* gamma,
                   const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                   float* scale, float* shift, float* mean, float* invstd, rvStream stream);
/* eval mode: scale/shift from the running statistics */
int rv_bn_fold_eval(int32_t c, const float* gamma, const float* beta, const float* running_mean,
                    const float* running_var, float eps, float* scale, float* shift, rvStream stream);

/* out = relu?( fa(a) + fb(b) ), f*(x) = relu?(scale*x + shift) per channel when the scale
 * pointer is non-NULL, identity otherwise; b may be NULL.  bf16 in / bf16 out.
 * Replaces `F.relu_(self.net(x) + residual)` (nn/blocks/__init__.py:81), `x_1 + x_2` after
 * BN+ReLU (:177-180) and standalone BatchNorm2d+ReLU applications. */
#define RV_EW_RELU_A 1
#define RV_EW_RELU_B 2
#define RV_EW_RELU_OUT 4
int rv_ew_combine(int64_t pixels, int32_t c, const void* a, int32_t ld_a, const float* a_scale,
                  const float* a_shift, const void* b, int32_t ld_b, const float* b_scale,
                  const float* b_shift, void* out, int32_t ld_out, int32_t flags, rvStream stream);

/* BatchNorm backward, fused with the ReLU masks around it.
 *   g  = dOut * [OUT > 0 if out != NULL] * [scale*y+shift > 0 if RV_BNB_RELU_Z]
 *   pass 1 (reduce): partial[rows][2][c] = (sum g, sum g*xhat), xhat = (y-mean)*invstd
 *   finalize       : dgamma = sum g*xhat, dbeta = sum g (accumulated into the fp32 grads),
 *                    coef[0][c] = gamma*invstd, coef[1][c] = mean(g), coef[2][c] = mean(g*xhat)
 *   pass 2 (apply) : dY = coef0 * (g - coef1 - xhat*coef2)  (bf16), and optionally
 *                    dRes (+)= g  (identity residual branch).
 * Replaces cuDNN BatchNorm backward + ReLU backward + the add's gradient fan-out.
 * Every pass here, rv_ew_combine and rv_ew_mask_grad reject, before any launch: pixels <= 0, c <= 0, c % 8, a row pitch that is
 * no multiple of 8 or below c (of a tensor that is given); the BatchNorm passes also c > 2048. */
#define RV_BNB_RELU_Z 1
#define RV_BNB_RES_ACCUM 2
#define RV_BNB_Y_FROM_INPUT 4 /* rv_bn_bwd_smallk*: y (may be NULL) is recomputed as W v from the conv input and w_packed */
int32_t rv_bn_bwd_rows(int64_t pixels);
int rv_bn_bwd_reduce(int64_t pixels, int32_t c, const void* dout, int32_t ld_dout, const void* out, int32_t ld_out,
                     const void* y, int32_t ld_y, const float* scale, const float* shift, const float* mean,
                     const float* invstd, int32_t flags, float* partial, rvStream stream);
/* The reduce pass for the TWO BatchNorms under one block sum out = relu(bn_a(ya) + bn_b(yb)) -- a BasicBlock with a projection
 * (nn/blocks/__init__.py:68-81: net(x) + projection_block(x)) -- in one launch: both take g = dOut * [out > 0]; partial_a /
 * partial_b receive (sum g, sum g * xhat_a) and (sum g, sum g * xhat_b) in rv_bn_bwd_reduce's layout ([rv_bn_bwd_rows(pixels) +
 * RV_STATS_SCRATCH_ROWS][2][c]).  Four tensor reads where two rv_bn_bwd_reduce launches take six. */
int rv_bn_bwd_reduce_pair(int64_t pixels, int32_t c, const void* dout, int32_t ld_dout, const void* out, int32_t ld_out,
                          const void* ya, int32_t ld_ya, const float* mean_a, const float* invstd_a, const void* yb, int32_t ld_yb,
                          const float* mean_b, const float* invstd_b, float* partial_a, float* partial_b, rvStream stream);
/* ... and their apply pass: dYa = coef_a0 * (g - coef_a1 - xhat_a * coef_a2), dYb likewise, g formed once (coef_* from
 * rv_bn_bwd_finalize over partial_a / partial_b).  Four reads and two writes where two rv_bn_bwd_apply launches take six and two. */
int rv_bn_bwd_apply_pair(int64_t pixels, int32_t c, const void* dout, int32_t ld_dout, const void* out, int32_t ld_out,
                         const void* ya, int32_t ld_ya, const float* mean_a, const float* invstd_a, const float* coef_a, void* dya,
                         int32_t ld_dya, const void* yb, int32_t ld_yb, const float* mean_b, const float* invstd_b,
                         const float* coef_b, void* dyb, int32_t ld_dyb, rvStream stream);
int rv_bn_bwd_finalize(const float* partial, int32_t rows, int32_t c, int64_t count, const float* gamma,
                       const float* invstd, float* dgamma, float* dbeta, int32_t accumulate, float* coef,
                       rvStream stream);
int rv_bn_bwd_apply(int64_t pixels, int32_t c, const void* dout, int32_t ld_dout, const void* out, int32_t ld_out,
                    const void* y, int32_t ld_y, const float* scale, const float* shift, const float* mean,
                    const float* invstd, const float* coef, int32_t flags, void* dy, int32_t ld_dy, void* dres,
                    int32_t ld_dres, rvStream stream);
/* Backward of a tower's FINAL 1x1 conv (c -> n_out <= 32 channels; nn/heads/dense_head.py:44-57, 74-76) fused with the BatchNorm
 * (+ReLU) backward of the conv -> BatchNorm -> ReLU unit in front of it: the input gradient dA = W^T dY (a K = 32 GEMM of the tiny
 * output gradient) is RECOMPUTED in both passes instead of being stored and read back twice --
 *   _sums : g = dA * [scale*y+shift > 0 if relu], partial[row][0][c] = sum g, partial[row][1][c] = sum g * (y-mean)*invstd over
 *           rv_head_final_bwd_rows(pixels) <= 512 pixel ranges (the rows rv_bn_bwd_finalize takes; + RV_STATS_SCRATCH_ROWS);
 *           dw_partial (may be NULL): [rows][32][c] fp32 partial WEIGHT gradients of the final conv, dW[o][c] = sum_px dY[px][o] *
 *           relu?(scale*y+shift)[px][c] over the row's pixels -- sum the rows in order (rv_reduce_rows with cols = 32 c) for the
 *           gradient in the parameter's own layout [n_out][c][1][1] (rows o >= n_out are zero)
 *   _apply: dy = coef0 * (g - coef1 - xhat * coef2)  (bf16; coef from rv_bn_bwd_finalize)
 * y: raw bf16 output of the unit's conv [pixels][ld_y]; dY: the final conv's output gradient as bf16 [pixels][ld_dy >= 32] with
 * channels n_out..31 zero; w_scatter: the final conv's packed scatter image ([c][32]); c % 256 == 0.
 * Replaces ATen conv2d backward-data + conv2d backward-weight + native_batch_norm_backward + threshold_backward for that pair of
 * layers (three transfers of a c-channel tensor instead of seven). */
int32_t rv_head_final_bwd_rows(int64_t pixels);
int rv_head_final_bwd_sums(int64_t pixels, int32_t c, const void* y, int32_t ld_y, const void* dY, int32_t ld_dy, const void* w_scatter,
                           const float* scale, const float* shift, const float* mean, const float* invstd, int32_t relu, float* partial,
                           float* dw_partial, rvStream stream);
int rv_head_final_bwd_apply(int64_t pixels, int32_t c, const void* y, int32_t ld_y, const void* dY, int32_t ld_dy, const void* w_scatter,
                            const float* scale, const float* shift, const float* mean, const float* invstd, int32_t relu, const float* coef,
                            void* dy, int32_t ld_out, rvStream stream);
/* Small-K layers whose input needs no gradient (1x1 conv with cin <= 8 followed by BatchNorm: the stem's 3 -> C positional
 * conv, the 5/6 -> C feature projections): BatchNorm backward AND the conv's weight gradient from one pass over
 * (dOut, y, v) -- dy is never written.  v = the conv input (bf16 NHWC, >= 8 stored channels), w_packed = the layer's packed
 * gather image (bf16 [c][ld_w]); dW is fp32 [c][cin].  Replaces cuDNN BatchNorm backward + conv2d backward-weight.
 * Precondition (cin_pad = 4 for cin <= 4, else 8): the per-pixel passes -- rv_bn_bwd_smallk / _sums with RV_BNB_Y_FROM_INPUT and
 * rv_smallk_forward's apply pass -- multiply ALL cin_pad columns of w_packed with the stored channels of v, so ld_w >= cin_pad,
 * the columns cin..cin_pad-1 of w_packed are zero (rv_pack_weight pads with zeros) and the channels cin..cin_pad-1 of v are finite
 * (any finite value; they also reach moms / moments and the planes R[d >= cin], which nothing reads).  The statistics pass of
 * rv_smallk_forward and rv_bn_bwd_smallk_from_sums read the columns below cin only, and the statistics pass the moments of the
 * channels below cin only. */
int64_t rv_bn_bwd_smallk_workspace_bytes(int64_t pixels, int32_t c, int32_t cin);
int rv_bn_bwd_smallk(int64_t pixels, int32_t c, const void* dout, int32_t ld_dout, const void* out, int32_t ld_out,
                     const void* y, int32_t ld_y, const float* scale, const float* shift, const float* mean,
                     const float* invstd, int32_t flags, const void* v, int32_t ld_v, int32_t cin, const void* w_packed,
                     int32_t ld_w, const float* gamma, const float* stat_mean, const float* stat_invstd, int64_t count,
                     float* dgamma, float* dbeta, float* dW, void* workspace, rvStream stream);
/* The same in two phases, for SyncBN: (A) this rank's sums -- sums[(2 + cin_pad) * c] = planes (sum g, sum g*xhat,
 * sum g*v_d), moms[cin_pad + cin_pad^2] = (sum v, sum v v^T) -- then the caller all-reduces sums[0 : 2c] into global_s01
 * and (B) forms the gradients (global_s01 == NULL: single rank). */
int rv_bn_bwd_smallk_sums(int64_t pixels, int32_t c, const void* dout, int32_t ld_dout, const void* out, int32_t ld_out,
                          const void* y, int32_t ld_y, const float* scale, const float* shift, const float* mean,
                          const float* invstd, int32_t flags, const void* v, int32_t ld_v, int32_t cin, const void* w_packed,
                          int32_t ld_w, double* sums, double* moms, void* workspace, rvStream stream);
int rv_bn_bwd_smallk_from_sums(int32_t c, int32_t cin, const double* sums, const double* moms, const double* global_s01,
                               const void* w_packed, int32_t ld_w, const float* gamma, const float* stat_mean,
                               const float* stat_invstd, int64_t count, float* dgamma, float* dbeta, float* dW,
                               rvStream stream);
/* Forward of the same layers: h = relu?(BatchNorm(W v)) as ONE element-wise pass; in training the batch statistics come
 * in closed form from the data moments (m1 = sum v, M2 = sum v v^T: rv_smallk_moments writes cin_pad + cin_pad^2 doubles,
 * cin_pad = 4 or 8; the caller all-reduces them under SyncBN), so neither the raw conv output nor a statistics pass over
 * it exists.  moments == NULL: eval, scale/shift are inputs (rv_bn_fold_eval).  h == NULL: statistics only (the caller
 * applies them itself: rv_pos_forward).  For the backward of such a layer call
 * rv_bn_bwd_smallk with RV_BNB_Y_FROM_INPUT (y = NULL: the raw output is recomputed from v, 16 bytes per pixel instead of
 * 2 C) and the layer's own scale / shift / mean / invstd; or, without the flag, with y = h, scale = 1, shift = 0,
 * mean = beta, invstd = 1/gamma, stat_* = the batch statistics (xhat rebuilt from the activated output).
 * Replaces cuDNN conv2d + BatchNorm + ReLU (nn/stems/__init__.py:40-57, nn/blocks/__init__.py:38-51 on 5/6-channel input). */
int64_t rv_smallk_forward_workspace_bytes(int32_t cin);
int rv_smallk_moments(const void* v, int32_t ld_v, int64_t pixels, int32_t cin, double* moments, void* workspace,
                      rvStream stream);
int rv_smallk_forward(const void* v, int32_t ld_v, int64_t pixels, int32_t cin, const void* w_packed, int32_t ld_w,
                      int32_t c, const double* moments, int64_t count, const float* gamma, const float* beta, float eps,
                      float momentum, float* running_mean, float* running_var, float* scale, float* shift, float* mean,
                      float* invstd, int32_t relu, void* h, int32_t ld_h, rvStream stream);
/* gradient of rv_ew_combine's plain (non-BN) inputs: d (+)= dOut * [OUT > 0 if out != NULL] */
int rv_ew_mask_grad(int64_t pixels, int32_t c, const void* dout, int32_t ld_dout, const void* out, int32_t ld_out,
                    void* d, int32_t ld_d, int32_t accumulate, rvStream stream);

/* Which kernel form a bandwidth-bound BatchNorm / element-wise pass launches for a shape (tests / bench labels; launches nothing).
 * The entry points launch from the very plan this reports.  pixels_or_rows: pixels, or the partial rows of a finalize pass;
 * ld: the row pitches (elements) as the entry point receives them, those of absent optional tensors included, in its argument order --
 * RV_EW_PASS_BWD_REDUCE {dout, out, y}, _REDUCE_PAIR {dout, out, ya, yb}, _BWD_APPLY {dout, out, y, dy, dres}; the other passes
 * do not read it; NULL = every pitch equals c;
 * has_out: the ReLU mask tensor `out` (RV_EW_PASS_COMBINE: the operand b) is given; has_dres: RV_EW_PASS_BWD_APPLY writes dres;
 * flags: RV_BNB_* of RV_EW_PASS_BWD_APPLY; finalize passes: non-zero = device-side count (count < 0).
 *   host_info[0] = form: RV_EW_FORM_COMB   grid-stride comb over channel octets (ew_combine_kernel, ew_mask_grad_kernel)
 *                        RV_EW_FORM_ROWS   one contiguous pixel range per workgroup (ew_combine_rows_kernel)
 *                        RV_EW_FORM_OCTET  thread = (pixel lane, channel octet), 64-bit addresses (bn_bwd_reduce_kernel, _reduce2_kernel,
 *                                          bn_bwd_apply_kernel, bn_bwd_apply2_kernel): c > 1024 or byte offsets of 2^32 and more
 *                        RV_EW_FORM_LEAN   thread = (pixel lane, channel quad), 32-bit byte offsets (bn_bwd_*_lean_kernel)
 *                        RV_EW_FORM_FUSED_FINALIZE  one launch sums the partial rows and finalises (at most 2048 rows)
 *                        RV_EW_FORM_TWO_STAGE       col_reduce_kernel into 64 fp64 group rows, then the finalize kernel
 *   host_info[1] = 1: non-temporal loads and stores (pixels * c * 2 bytes reach 256 MiB)
 *   host_info[2] = workgroups (of the second launch for RV_EW_FORM_TWO_STAGE)
 *   host_info[3] = template argument of the instantiation: RV_EW_PASS_BWD_APPLY lean: F of bn_bwd_apply_lean_kernel<F> (1 non-temporal
 *                  | 2 out | 4 dres | 8 RV_BNB_RES_ACCUM), octet and RV_EW_PASS_BWD_APPLY_PAIR: MODE; RV_EW_PASS_BWD_REDUCE lean: OUT;
 *                  RV_EW_PASS_COMBINE rows: HAS_B; finalize passes: 1 = device-side count; 0 otherwise. */
#define RV_EW_PASS_COMBINE 0
#define RV_EW_PASS_MASK_GRAD 1
#define RV_EW_PASS_BN_FINALIZE 2
#define RV_EW_PASS_BWD_REDUCE 3
#define RV_EW_PASS_BWD_REDUCE_PAIR 4
#define RV_EW_PASS_BWD_FINALIZE 5
#define RV_EW_PASS_BWD_APPLY 6
#define RV_EW_PASS_BWD_APPLY_PAIR 7
#define RV_EW_FORM_COMB 1
#define RV_EW_FORM_ROWS 2
#define RV_EW_FORM_OCTET 3
#define RV_EW_FORM_LEAN 4
#define RV_EW_FORM_FUSED_FINALIZE 5
#define RV_EW_FORM_TWO_STAGE 6
int rv_ew_pass_info(int32_t pass, int64_t pixels_or_rows, int32_t c, const int32_t* ld, int32_t has_out, int32_t has_dres,
                    int32_t flags, int32_t* host_info);

/* RangePartition stem (nn/stems/__init__.py:88-135, the stem RangeNet builds for stem_type RANGE_PARTITION, nn/backbones/dla.py:164-171):
 * `features = (partitions[:, :, None] * features[:, None]).flatten(1, 2) * mask` with partitions = (||cart|| >= lower) & (||cart|| <= upper)
 * as the 16-bit NHWC operand of the projecting BasicBlock -- channel band * C + c, zeros in the padding channels.  features / cart fp32
 * NCHW, mask one byte per pixel; `lower` / `upper`: `bands` host floats (the module's lower_bounds / upper_bounds parameters). */
int rv_range_partition(const float* features_nchw, const float* cart_nchw, const uint8_t* mask, int32_t N, int32_t C, int32_t H, int32_t W,
                       const float* lower, const float* upper, int32_t bands, void* dst, int32_t ld_dst, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Layout conversion at the module boundary (the reference's tensors are NCHW fp32).
 * ------------------------------------------------------------------------------------- */
int rv_nchw_f32_to_nhwc_bf16(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, void* dst, int32_t ld_dst,
                             int32_t c_offset, rvStream stream);
int rv_nhwc_bf16_to_nchw_f32(const void* src, int32_t ld_src, int32_t c_offset, int32_t N, int32_t C, int32_t H,
                             int32_t W, float* dst, rvStream stream);
int rv_nhwc_f32_to_nchw_f32(const float* src, int32_t ld_src, int32_t N, int32_t C, int32_t H, int32_t W, float* dst,
                            rvStream stream);
int rv_nchw_f32_to_nhwc_f32(const float* src, int32_t N, int32_t C, int32_t H, int32_t W, float* dst, int32_t ld_dst,
                            rvStream stream);

/* ---------------------------------------------------------------------------------------
 * MetaKernel stem (nn/stems/__init__.py:64-85): F.unfold of features and of `cart`,
 * relative coordinates, positional MLP, element-wise product.  The 9x unfolded tensors of
 * the reference are never written to memory.
 * ------------------------------------------------------------------------------------- */
/* rel[n,h,w,tap,0:3] = cart[n,h+dy,w+dx,:] (0 outside) - cart[n,h,w,:], written as a bf16
 * NHWC tensor (N, H, W*9, 32) whose channels 3..31 are zero (operand of the 3->C 1x1 conv).
 * `cart` is NCHW fp32 (B,3,H,W) exactly as the reference's batch dict holds it. */
int rv_meta_relative(const float* cart_nchw, int32_t N, int32_t H, int32_t W, void* rel, rvStream stream);
/* geo[n,h,w, tap*C + c] = relu(scale[c]*pos[n,h,w,tap,c] + shift[c]) * feat[n,h+dy,w+dx,c]
 * (zero outside the image).  The reference's channel order c*9+tap (F.unfold) is absorbed
 * into the packed weight of the 9C->C fusion conv. */
int rv_meta_modulate(const void* pos_raw, const float* scale, const float* shift, const void* feat, int32_t ld_feat,
                     int32_t N, int32_t H, int32_t W, int32_t C, void* geo, rvStream stream);
/* backward of rv_meta_modulate: dpos_act = dgeo * feat_nbr (then ReLU/BN backward via
 * rv_bn_bwd_*), dfeat[n,h',w',c] += sum_tap dgeo * pos_act. */
int rv_meta_modulate_bwd(const void* dgeo, const void* pos_raw, const float* scale, const float* shift,
                         const void* feat, int32_t ld_feat, int32_t N, int32_t H, int32_t W, int32_t C,
                         void* dpos_act, void* dfeat, int32_t ld_dfeat, rvStream stream);
/* The same backward FUSED with the BatchNorm(+ReLU) backward of the positional layer whose output `pos_raw` is
 * (training path; nn/stems/__init__.py:80-84 differentiated through Conv2dNormActivation's BatchNorm2d + ReLU):
 *   z = dgeo * feat_nbr * [relu passed]  (never written),  S0 = sum z, S1 = sum z*xhat,  dfeat as above.
 * _sums: one pass over (dgeo, pos_raw): dfeat and rv_meta_bwd_rows(N,H,W) partial rows [row][2][C] of (S0, S1) in the
 *        layout rv_bn_bwd_finalize reads (allocate rows + RV_STATS_SCRATCH_ROWS).
 * _apply: dy[n,h,w,tap,c] = coef0 (z - coef1 - xhat coef2) with `coef` from rv_bn_bwd_finalize.
 * Two passes over the 9x-grid tensors instead of four, and z stays in registers. */
int32_t rv_meta_bwd_rows(int32_t N, int32_t H, int32_t W);
int rv_meta_modulate_bwd_sums(const void* dgeo, const void* pos_raw, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const void* feat, int32_t ld_feat, int32_t N,
                              int32_t H, int32_t W, int32_t C, void* dfeat, int32_t ld_dfeat, float* partial,
                              rvStream stream);
int rv_meta_modulate_bwd_apply(const void* dgeo, const void* pos_raw, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const float* coef, const void* feat,
                               int32_t ld_feat, int32_t N, int32_t H, int32_t W, int32_t C, void* dy, rvStream stream);

/* The two positional layers of the MetaKernel stem (nn/stems/__init__.py:41-49, 80: Conv2dNormActivation(3, C, 1) ->
 * Conv2dNormActivation(C, C, 1) on the 9x neighbour grid) as ONE persistent streaming GEMM, C = 256 (rv-av2) or 128 (rv-waymo):
 *   h1 = relu(scale1 * (W1 rel) + shift1)   generated in the K-operand staging from `rel` (bf16 [pixels][ld_rel], cin <= 3
 *                                           channels used) and written once (the second layer's weight gradient reads it),
 *   y2 = W2 h1                              raw bf16, with fp32 (sum, sum of squares) rows of the accumulators in
 *                                           stats_partial [rv_pos_forward_rows(pixels) + RV_STATS_SCRATCH_ROWS][2][C] (NULL: eval).
 * scale1 / shift1: the first layer's folded BatchNorm (rv_smallk_forward with h == NULL forms them in closed form).
 * Replaces rv_smallk_forward's apply pass + rv_tap_gather of the second layer (cuDNN conv2d x2 + BatchNorm + ReLU). */
int32_t rv_pos_forward_rows(int64_t pixels);
int rv_pos_forward(const void* rel, int32_t ld_rel, int32_t cin, int64_t pixels, const void* w1_packed, int32_t ld_w1,
                   const float* scale1, const float* shift1, const void* w2_packed, int32_t c, void* h1, void* y2,
                   float* stats_partial, rvStream stream);

/* Inference form of the same kernel with the modulation of MetaKernel.forward (nn/stems/__init__.py:80-83: positional
 * weights times the unfolded neighbour features) in its epilogue: row 9 p + k of the 9x grid is neighbour k of pixel p, and
 *   geo[p][k*c + ch] = relu(scale2[ch] * y2[9 p + k][ch] + shift2[ch]) * feat[neighbour k of p][ch]   (0 outside the image)
 * is what the kernel stores -- neither h1 nor y2 reaches memory (2 x 2.4 GB at 4 x 64 x 2048 x 256), and the separate
 * rv_meta_modulate pass (read 2.4 GB, write 2.4 GB) disappears.  y2 is rounded to the storage type before the BatchNorm, as the
 * stored tensor was: the result equals rv_pos_forward + rv_meta_modulate bit for bit.  scale2 / shift2: the second layer's
 * eval-mode BatchNorm (rv_bn_fold_eval); feat: bf16/fp16 [N*H*W][ld_feat]; geo: [N*H*W][9*c].  W >= 32, 9 N H W < 2^31. */
int rv_pos_modulate_forward(const void* rel, int32_t ld_rel, int32_t cin, const void* w1_packed, int32_t ld_w1, const float* scale1,
                            const float* shift1, const void* w2_packed, int32_t c, const float* scale2, const float* shift2,
                            const void* feat, int32_t ld_feat, int32_t N, int32_t H, int32_t W, void* geo, rvStream stream);

/* Backward of the same pair: the second layer's backward-data GEMM dh1 = dy2 W2 fused with phase (A) of the first layer's
 * small-K BatchNorm backward (rv_bn_bwd_smallk_sums with RV_BNB_Y_FROM_INPUT): dh1 is consumed in registers and never
 * written -- 2.4 GB less to store and 2.4 GB less to read back at 4 x 64 x 2048.  w2_scatter = the second layer's packed
 * scatter image; sums / moms / workspace as rv_bn_bwd_smallk_sums (cin_pad = 4); continue with rv_bn_bwd_smallk_from_sums.
 * Replaces rv_tap_scatter of the second layer + rv_bn_bwd_smallk_sums of the first (ATen conv backward-data + BatchNorm
 * backward + conv backward-weight). */
int rv_pos_backward_sums(int64_t pixels, int32_t c, const void* dy2, const void* w2_scatter, const void* rel, int32_t ld_rel,
                         int32_t cin, const void* w1_packed, int32_t ld_w1, const float* scale1, const float* shift1,
                         const float* mean1, const float* invstd1, double* sums, double* moms, void* workspace, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Optimiser step of the recipe (nn/meta/arch.py:57 -> torch.optim.AdamW via conf/model/range_view.yaml:52-55; gradient
 * clipping = Lightning's gradient_clip_val 35.0, conf/trainer/train.yaml) for ALL parameters in two launches.
 * tensors: n_tensors x {float* p; const float* g; float* m; float* v; int64 n} (device table), chunks: n_chunks x
 * {int32 tensor; int32 chunk} with chunk < ceil(n / rv_optim_chunk_elems()), partial: n_chunks floats of scratch.
 * Arithmetic = torch/optim/adamw.py (foreach, non-capturable) in fp32, `step` = the 1-based step count of the bias
 * corrections; max_norm > 0: g is scaled by min(1, max_norm / (||g||_2 + 1e-6)) on the fly (torch.nn.utils.clip_grad_norm_;
 * the stored gradients stay untouched), total_norm (optional) receives ||g||_2.
 * Replaces ATen's foreach norm / mul / lerp / addcmul / sqrt / div / addcdiv launches.
 * ------------------------------------------------------------------------------------- */
int32_t rv_optim_chunk_elems(void);
int rv_adamw_step(const void* tensors, const void* chunks, int32_t n_chunks, float* partial, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int64_t step, double max_norm, float* total_norm,
                  rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Decoder (nn/decoders/range_decoder.py:29-156, math/ops/coding.py:79-144,
 * math/linalg/lie/SO3.py:122-134).
 * ------------------------------------------------------------------------------------- */
/* Per pixel: score = max_c sigmoid(logit_c)*mask (ties -> lowest class), category = argmax,
 * box = decode_range_view(regressands, cart) evaluated in fp64 and rounded to fp32.
 * Inputs are NCHW fp32 (the module boundary layout).  With `n_bands` > 0 the outputs are
 * written in sample_by_range order: K = H * sum_i ceil(W / rate_i) candidates per sweep,
 * band-major; scores are zeroed outside the band (lower, upper], boxes/categories are not.
 * With n_bands == 0 the outputs are the dense H*W grid.
 *   scores (B,K) f32, categories (B,K) i64, boxes (B,K,7) f32. */
int rv_decode_candidates(const float* logits, const float* regressands, const float* cart, const uint8_t* mask,
                         int32_t B, int32_t n_cls, int32_t H, int32_t W, int32_t azimuth_invariant, int32_t n_bands,
                         const float* host_lower, const float* host_upper, const int32_t* host_rates,
                         int64_t category_offset,
                         float* scores, int64_t* categories, float* boxes, rvStream stream);
int64_t rv_decode_num_candidates(int32_t H, int32_t W, int32_t n_bands, const int32_t* host_rates);
/* decode_range_view alone on NCHW fp32 (B,8,H,W)+(B,3,H,W) -> (B,7,H,W) (math/ops/coding.py:110-144) */
int rv_decode_range_view(const float* regressands, const float* cart, int32_t B, int32_t H, int32_t W,
                         int32_t azimuth_invariant, float* out, rvStream stream);
/* yaw (n,) -> wxyz quaternions (n,4)  (SO3.py:122-134) */
int rv_yaw_to_quat(const float* yaw, int64_t n, int64_t yaw_stride, float* quat, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Weighted NMS -- replaces `weighted_nms_ext.wnms_gpu(boxes, data2merge_score, output, keep,
 * count, nms_thresh, merge_thresh, device_index) -> int` (math/ops/nms.py:161-170).
 * Same contract: inputs sorted by score descending; boxes (n,5) = [x1,y1,x2,y2,ry] f32;
 * data (n,d) f32 with the score in the last column; caller-allocated zero-initialised
 * `output` (n,d), `keep` (n,) i64, `count` (n,) i64 -- all DEVICE buffers here (the
 * reference keeps `keep` on the host); returns the number of kept boxes through
 * `host_num_out` after synchronising `stream` (the reference call is synchronous too).
 * `workspace`: rv_wnms_workspace_bytes(n) bytes.  Semantics: see oracle/nms.py (the
 * third-party kernel's arithmetic is not in the reference tree -- parity unpinned).
 * ------------------------------------------------------------------------------------- */
int64_t rv_wnms_workspace_bytes(int64_t n);
int rv_wnms(const float* boxes, const float* data, int64_t n, int32_t d, float nms_thresh, float merge_thresh,
            float* output, int64_t* keep, int64_t* count, void* workspace, int64_t* host_num_out, rvStream stream);
/* The same with a class id per box (cats, i32, may be NULL): boxes of different classes neither suppress nor merge, so ONE
 * call does what the reference's per-class loop does (weighted_multiclass_nms, math/ops/nms.py:64-123) -- identical rows
 * per class, since classes do not interact and the score order within a class is preserved. */
int rv_wnms_classes(const float* boxes, const float* data, const int32_t* cats, int64_t n, int32_t d, float nms_thresh,
                    float merge_thresh, float* output, int64_t* keep, int64_t* count, void* workspace,
                    int64_t* host_num_out, rvStream stream);
/* The declared choices as PER-CALL options (the library keeps no option state).  oracle/nms.py declares the semantics because the
 * third-party kernel's source is absent; the declaration contains four free choices, and these four are the axes along which a
 * third-party `wnms_gpu` may differ from the declaration.  A clear bit is the declaration (what rv_wnms / rv_wnms_classes /
 * rv_nms_sweeps compute); a set bit is the other reading:
 *   RV_WNMS_MERGE_SUPPRESSED  merge set: the cluster of kept box i is i plus EVERY later box j > i of its class whose IoU with i
 *                             passes the merge test, whether or not j was suppressed before i was visited -- a box may be a
 *                             member of several clusters, and `count` follows the cluster.  Clear: only the boxes not yet
 *                             suppressed at i's visit.  Suppression itself is the same.
 *   RV_WNMS_SCORE_KEEPER      score column: the LAST column of an output row is the kept box's own score, data[i][d-1], copied bit
 *                             for bit; the other d-1 columns stay the score-weighted means.  Clear: the last column is the weighted
 *                             mean too (sum s^2 / sum s).  In the batch entry the per-class top-k then ranks by the kept scores.
 *   RV_WNMS_NMS_GE            a kept box suppresses a later box when iou >= nms_thresh.  Clear: iou > nms_thresh.
 *   RV_WNMS_MERGE_GE          a box joins a cluster when iou >= merge_thresh.  Clear: iou > merge_thresh.
 * Members are visited in ascending index order under every setting (fixed summation order).  With a `>=` test against a threshold
 * <= 0 every pair of a class passes, far-apart pairs (IoU 0) included.  Which setting a given third-party build is stays unpinned
 * until its `wnms_gpu` is run through tests/tools/pin_wnms.py.
 *
 * rv_wnms_opt: the arguments of rv_wnms_classes (cats may be NULL) and `flags`; rv_nms_sweeps_opt (below): those of rv_nms_sweeps
 * and `flags`.  Same workspaces, same `resume` / `out_counts` protocol, same launches; flags = 0 is rv_wnms_classes /
 * rv_nms_sweeps bit for bit (those entries are calls of these).  A bit outside the four fails (rv_last_error). */
#define RV_WNMS_MERGE_SUPPRESSED 1
#define RV_WNMS_SCORE_KEEPER 2
#define RV_WNMS_NMS_GE 4
#define RV_WNMS_MERGE_GE 8
/* The two prototypes live in include/rv3d_wnms.h, which this line makes part of this header (a C / C++ caller needs rv3d.h only):
 * this file's own list of prototypes stays the list that the binding's census counts, and the binding (`_lib.py`) types the entries
 * of an included header exactly as it types this file's. */
#include "rv3d_wnms.h"
/* pairwise rotated BEV IoU (n x m), exposed for tests */
/* The whole post-decode path of a BATCH of sweeps, device-resident from end to end (csrc/nms2.hip): confidence filter +
 * compaction, (class, score) ordering, class-segmented weighted NMS (one scan workgroup per class), per-class top-k by
 * merged score, final compaction in the reference's output order (math/ops/nms.py:64-123, 181-266: sweeps in order, classes
 * ascending, merged score descending).  scores (B,K) f32, cats (B,K) i64 in [0, n_classes), cuboids (B,K,7) f32
 * [x,y,z,l,w,h,yaw]; `cap` = candidate capacity per sweep (multiple of 64, <= 262144: the decoder emits 212 992 per
 * 64 x 2048 sweep; per-candidate workspace: rv_nms_sweeps_workspace_bytes, ~117 bytes per candidate).  The pair masks are
 * class-relative and live in `mask_workspace`: B x 2 x `mask_words` 64-bit words; a sweep whose classes need more than
 * `mask_words` (= sum over classes of n_c * ceil(n_c / 64), n_c cut at num_pre_nms: the reference's per-class pre-NMS top-k,
 * nms.py:83-84) reports the number and is redone by a call with `resume` != 0 over a buffer of that size (the ordering
 * stages are not repeated; `workspace` must be untouched in between).  Outputs (device): out_boxes (B,out_cap,7),
 * out_scores (B,out_cap), out_cats (B,out_cap), out_cap >= min(cap, n_classes * num_post_nms);
 * out_counts (B,4) i64 = {rows written, or -1: mask budget exceeded, -2: more than `cap` candidates;
 * candidates >= min_confidence; boxes kept by the NMS; mask words the sweep needs}.
 * Asynchronous: the caller reads out_counts back once for the whole batch. */
int64_t rv_nms_sweeps_workspace_bytes(int32_t B, int32_t cap);
int rv_nms_sweeps(const float* scores, const int64_t* cats, const float* cuboids, int32_t B, int64_t K, int32_t n_classes,
                  float min_confidence, float nms_thresh, float merge_thresh, int32_t num_pre_nms, int32_t num_post_nms,
                  int32_t cap, int32_t out_cap, float* out_boxes, float* out_scores, int32_t* out_cats, int64_t* out_counts,
                  void* workspace, void* mask_workspace, int64_t mask_words, int32_t resume, rvStream stream);
/* ---------------------------------------------------------------------------------------
 * Hard NMS (`post_processing_config.nms_mode: HARD`) -- replaces `detectron2.layers.nms.nms_rotated(boxes, scores,
 * iou_threshold) -> keep` as `hard_multiclass_nms` uses it (math/ops/nms.py:10-61) and, for a batch, that function's
 * per-class loop inside `batched_multiclass_nms` (:181-266).  detectron2 is not part of the reference tree, so the last bit
 * of its IoU is not pinned (parity unpinned at the last bit of the IoU, as for rv_wnms); declared semantics:
 *   1. boxes are visited in descending score order (ties: ascending input index); a box not yet suppressed is kept;
 *   2. a kept box suppresses every later box whose rotated BEV IoU with it is STRICTLY GREATER than `iou_threshold`;
 *      a suppressed box suppresses nothing;
 *   3. the IoU is rv_rotated_iou's (rectangle [x1,y1,x2,y2,ry], unfused fp32, sin / cos = fp32 roundings of the fp64
 *      values).  detectron2 puts a box's width axis at (cos a, -sin a) -- `angle` runs counter-clockwise in IMAGE
 *      coordinates, y pointing down -- and the reference passes `-yaw` in degrees (nms.py:39): the rectangle whose length
 *      axis lies at +yaw, which is the one rv_nms_sweeps builds from the cuboid ([x - l/2, y - w/2, x + l/2, y + w/2, yaw]).
 *      The batch entry builds it that way, never through degrees.
 * Hard NMS is a SELECTION: every output row of rv_nms_sweeps_hard is a row of `cuboids` / `scores`, bit for bit.
 *
 * rv_nms_rotated -- one score-sorted list (the counterpart of rv_wnms_classes): boxes (n,5) = [x1,y1,x2,y2,ry] f32 sorted by
 * score descending, `cats` (n,) i32 or NULL (boxes of different classes do not suppress each other); writes the sorted
 * positions of the kept boxes, ascending, to `keep` (n,) i64 -- a DEVICE buffer owned by the caller, as is `workspace`
 * (rv_nms_rotated_workspace_bytes(n) bytes) -- and returns their number through `host_num_out` after synchronising `stream`.
 *
 * rv_nms_sweeps_hard -- the device-resident batch path: the arguments, the `resume` / `out_counts` protocol and the
 * per-candidate `workspace` (rv_nms_sweeps_workspace_bytes) of rv_nms_sweeps, without `merge_thresh`; there is ONE pair mask,
 * so `mask_workspace` is B x `mask_words` 64-bit words.  Rows per sweep: classes ascending, score descending (ties:
 * candidate index ascending), at most num_post_nms per class of the at most num_pre_nms best candidates of the class.
 * Asynchronous. */
int64_t rv_nms_rotated_workspace_bytes(int64_t n);
int rv_nms_rotated(const float* boxes, const int32_t* cats, int64_t n, float iou_threshold, int64_t* keep, void* workspace,
                   int64_t* host_num_out, rvStream stream);
int rv_nms_sweeps_hard(const float* scores, const int64_t* cats, const float* cuboids, int32_t B, int64_t K, int32_t n_classes,
                       float min_confidence, float iou_threshold, int32_t num_pre_nms, int32_t num_post_nms, int32_t cap,
                       int32_t out_cap, float* out_boxes, float* out_scores, int32_t* out_cats, int64_t* out_counts, void* workspace,
                       void* mask_workspace, int64_t mask_words, int32_t resume, rvStream stream);
int rv_rotated_iou(const float* a, int64_t n, const float* b, int64_t m, float* out, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Range-image projection (converters/av2/utils.py:108-208 == math/numpy/conversions.py:9-128).
 * ------------------------------------------------------------------------------------- */
/* Raw sweep -> the points the projection bins (converters/av2/utils.py:211-295, :32-55).  All device pointers.
 * rv_unmotion_compensate: xyz (n,3) fp64 ego-frame points of the sweep stamped `sweep_timestamp_ns` with per-point
 *   `offset_ns`; the pose track (sorted timestamps, wxyz quaternions, translations; `target_pose` = index of the pose at the
 *   sweep timestamp).  kept[i] = 0 for points outside (first, last) pose time (the reference drops them; their xyz_p is 0);
 *   xyz_p = the point in the ego frame AT ITS OWN capture time (scipy-Slerp rotation, the reference's translation weights).
 * rv_correct_laser_numbers: laser ids -> image rows through LASER_MAPPING (only for `affected` logs) and the row table
 *   (ROW_MAPPING_64 / _32 of datasets/argoverse/constants.py, passed in as data); ids outside the table give -1.
 * rv_se3_inverse_apply: out = R(q)^T (xyz - t): ego -> sensor with the sensor's extrinsics (egovehicle_SE3_sensor); points with
 *   kept[i] == 0 (kept may be NULL) come out as the origin: range 0, which rv_z_buffer skips -- the point order is preserved. */
int rv_unmotion_compensate(const double* xyz, const int32_t* offset_ns, int64_t n, int64_t sweep_timestamp_ns,
                           const int64_t* pose_timestamps_ns, const double* pose_q_wxyz, const double* pose_t, int32_t n_poses,
                           int32_t target_pose, double* xyz_p, uint8_t* kept, rvStream stream);
int rv_correct_laser_numbers(const int32_t* laser, int64_t n, int32_t affected, const int32_t* laser_mapping_32,
                             const int32_t* row_mapping, int32_t n_rows, int32_t* out, rvStream stream);
int rv_se3_inverse_apply(const double* xyz, int64_t n, const double* q_wxyz, const double* t, const uint8_t* kept, double* out,
                         rvStream stream);
/* Correctly rounded (round-to-nearest-even) fp64 atan2, elementwise -- the azimuth rv_project_indices bins with
 * (np.arctan2 at converters/av2/utils.py:172; see csrc/project.hip for why the device value must be THE rounded one). */
int rv_atan2_cr(const double* y, const double* x, int64_t n, double* out, rvStream stream);
/* fp64 hypot with the bits of the C library the reference runs on (np.hypot at math/numpy/conversions.py:64-65 ==
 * glibc 2.35 hypot: Borges' corrected sqrt, not correctly rounded) -- the range rv_project_indices returns and the
 * z-buffer compares (csrc/project.hip). */
int rv_hypot_libc(const double* x, const double* y, int64_t n, double* out, rvStream stream);
/* cart (n,3) f64 -> rows/cols (i32) + range (f64); variant 0 = converter binning
 * (col = W - round((az+pi)*W/tau)), 1 = library binning (col = round(W - (az+pi)*W/tau - 1));
 * round-half-to-even, clip to [0, W-1] before the integer cast; row = H - laser_mapping[laser] - 1. */
int rv_project_indices(const double* cart, const int32_t* laser, const int32_t* laser_mapping, int64_t n,
                       int32_t H, int32_t W, int32_t variant, int32_t* rows, int32_t* cols, double* range,
                       rvStream stream);
/* z-buffer with the reference's sequential semantics: skip range < min_range; pixel owner =
 * the point with the smallest float(range) ... see DESIGN.md §z-buffer for the exact rule
 * (fp64-vs-fp32 comparison, earliest index on ties).  features (c,n) f64 -> image (c,H,W) f32
 * (zeros where empty); winner (H,W) i64 (-1 where empty); `keys` is an (H*W) u64 scratch. */
int rv_z_buffer(const int32_t* rows, const int32_t* cols, const double* range, const double* features, int64_t n,
                int32_t c, int32_t H, int32_t W, double min_range, uint64_t* keys, float* image, int64_t* winner,
                rvStream stream);

/* Spherical <-> Cartesian (math/conversions.py:28-81, math/numpy/conversions.py:46-103): (n,3) arrays,
 * [azimuth, inclination, radius] <-> [x, y, z]; is_f64 selects double (numpy twins) or float (torch versions). */
int rv_cart_to_sph(const void* cart, int64_t n, int32_t is_f64, void* sph, rvStream stream);
int rv_sph_to_cart(const void* sph, int64_t n, int32_t is_f64, void* cart, rvStream stream);
/* The loader's per-sweep contract (prototype/loader.py:568-705, DataLoader.__getitem__): a range-view table with H*W rows
 * and named fp32 columns (`table`: [n_cols][hw], one column after the other, as Arrow stores it) -> features [n_feat][hw]
 * (= (F,H,W)), cart [3][hw], mask [hw] (range > 0).  roi_col >= 0: every column is first multiplied by that 0/1 column
 * (`filter_roi`, loader.py:599-601).  host_feat_op[f]: 0 copy, 1 tanh (Waymo intensity, :627), 2 times 1e-9 (timedelta_ns, :633).
 * The index arrays are HOST arrays (<= 16 features).  Replaces the polars select / to_numpy / transpose / reshape chain. */
int rv_table_to_range_view(const float* table, int32_t n_cols, int64_t hw, int32_t n_feat, const int32_t* host_feat_col,
                           const int32_t* host_feat_op, const int32_t* host_cart_col, int32_t range_col, int32_t roi_col,
                           float* features, float* cart, uint8_t* mask, rvStream stream);

/* Loader augmentations on device (prototype/loader.py:825-990: flip_azimuth, random_rotation, random_global_scale,
 * random_global_translation, and chains of them).  in / out: (B, C, H, W) fp32, distinct buffers.  params: B x 32 doubles
 * on the DEVICE: {a, b} column map w_src = (a*w + b) mod W with a = +-1; A[9], t[3] affine map of the channels ix / iy / iz
 * (xyz' = A xyz + t, fp64, rounded once); Ar[9], tr[3], use_range: the channel `irange` becomes ||Ar xyz + tr|| when
 * use_range != 0 (the reference recomputes the range only in random_global_scale); 5 pad doubles.  ix = iy = iz = -1: only the
 * column map is applied (mask, extra feature maps).  Every other channel is copied through the column map bit for bit. */
int rv_augment(const float* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ix, int32_t iy, int32_t iz,
               int32_t irange, const double* params, rvStream stream);
/* rv_augment with a `point_dropout` inside the chain (prototype/loader.py:506-512 `_point_dropout`, applied at its position in
 * `augmentations_config` by apply_augmentations, :514-549).  `params` as rv_augment (the whole chain); `post_params`: the same 32-double
 * layout for the steps AFTER the dropout only (a_post, b_post, A_post, t_post, Ar_post, tr_post, use_range_post = a
 * random_global_scale follows the dropout).  keep (B, H*W) u8 in the frame of the dropout step: the output pixel (h, w) looks at
 * keep[h * W + (a_post * w + b_post) mod W].  A kept pixel gets exactly what rv_augment gives it.  A dropped pixel is an empty pixel
 * from that step on: 0 in every non-Cartesian channel, A_post 0 + t_post in x / y / z and, in the `irange` channel,
 * ||Ar_post 0 + tr_post|| when use_range_post != 0 (else 0). */
int rv_augment_dropout(const float* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t ix, int32_t iy, int32_t iz,
                       int32_t irange, const double* params, const double* post_params, const uint8_t* keep, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Object-database sampling, "GT paste" (prototype/loader.py:708-789 `sample_database`, called from DataLoader.__getitem__ :672-682
 * on the UNPADDED image, after the augmentations and before subsample_range_view).  The database is one CSR block on the device:
 * points (P, 3 + F) fp32 = x, y, z, then the F feature columns; range (P) fp32 (>= 0); index (P) i32 = flat pixel h * W + w;
 * offsets (n_obj + 1) i64.  samples (B, S) i32: object id per (sweep, slot), -1 = empty slot; keep (B, S) u8: the verdict of the
 * collision steps (:726-733, through rv_rotated_iou).
 *
 * rv_db_paste_keys -- :741-742 (concat in sample order, sort by range, unique("index", keep="first")): the nearest point wins each
 *   pixel.  One unit of work per (sweep, slot, point) of the kept slots, listed by a prefix sum over their point counts;
 *   atomicMin(keys[b][index], float_bits(range) << 32 | work index).  TIE RULE: equal ranges on one pixel go to the lower
 *   (slot, point) position (the reference leaves them to an unstable sort).  The library initialises the keys and clears `owned`
 *   (B, S) u8.  `index_max`: the largest index of the block (checked against H * W here, on the host; the kernel also skips an index
 *   outside the image); `max_work`: an upper bound of the batch's point count (sizes the grid; < 2^32).  workspace:
 *   rv_db_paste_workspace_bytes(B, S, H, W) bytes, handed on to rv_db_paste_resolve.  Two launches.
 * rv_db_paste_resolve -- :744-772, one pass over the B * H * W pixels, in -> out (distinct buffers): a pixel whose key was taken
 *   gets its winner's F features, x / y / z in `cart` and mask = sqrtf(x*x + y*y + z*z) > 0 (fp32, :756) and sets owned[b][slot] = 1
 *   (:744-745: a sample that owns no pixel leaves the annotations); EVERY pixel leaves with features * mask (:772).  A pasted point
 *   overwrites the scene's pixel: there is no depth test against the scene.  mask: u8 0 / 1.  One launch.
 * Both are asynchronous. */
int64_t rv_db_paste_workspace_bytes(int32_t B, int32_t S, int32_t H, int32_t W);
int rv_db_paste_keys(const int32_t* samples, const uint8_t* keep, int32_t B, int32_t S, const int64_t* offsets, int64_t n_obj,
                     const float* range, const int32_t* index, int64_t index_max, int64_t max_work, int32_t H, int32_t W,
                     uint8_t* owned, void* workspace, rvStream stream);
int rv_db_paste_resolve(const float* features_in, const float* cart_in, const uint8_t* mask_in, float* features_out, float* cart_out,
                        uint8_t* mask_out, int32_t B, int32_t F, int32_t H, int32_t W, const int32_t* samples, int32_t S,
                        const int64_t* offsets, const float* points, const void* workspace, uint8_t* owned, rvStream stream);
/* The database BUILDER's kernel (the reference ships none; the layout is what `sample_database` reads): for every row of `cuboids` /
 * `box_offsets` (as rv_assign_targets) the pixels of its sweep with mask != 0 that lie inside the cuboid -- the interior test of
 * rv_assign_targets (compute_interior_points_mask, math/polytope.py:14-56).  out_index == NULL: count pass and scan, counts (m) i64
 * and obj_offsets (m + 1) i64 are written; out_index != NULL (capacity entries, >= obj_offsets[m]): fill pass, object k's flat
 * pixel indices at obj_offsets[k] .. obj_offsets[k + 1], ascending (independent of scheduling).  A pixel inside two overlapping
 * cuboids belongs to both objects.  mask: u8 (B, H*W).  Asynchronous. */
int rv_db_extract(const float* cart, const uint8_t* mask, int32_t B, int32_t H, int32_t W, const double* cuboids, int32_t m,
                  const int32_t* box_offsets, int64_t* counts, int64_t* obj_offsets, int32_t* out_index, int64_t capacity, rvStream stream);

/* subsample_range_view's W padding at x_stride 1 (prototype/loader.py:792-815): out (C,H,W+2*pad) = pad(image * mask);
 * mask (H,W) may be NULL; circular != 0 wraps around in azimuth, else zeros.  AV2 pad 4 (1800 -> 1808), Waymo 3. */
int rv_pad_range_view(const float* image, const float* mask, int32_t C, int32_t H, int32_t W, int32_t pad,
                      int32_t circular, float* out, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Targets + losses on device (nn/heads/detection_head.py:496-665, math/ops/assignment.py:76-161,
 * nn/functional/__init__.py:8-27, detection_head.py:202-449) -- see rv3d.h section in DESIGN.md.
 * ------------------------------------------------------------------------------------- */
/* cuboids (m,10) f64 [x,y,z,l,w,h,yaw,task,category,batch] grouped by sweep; `box_offsets` (B+1) i32 is the
 * CSR of the grouping (device); cart NCHW f32.  Outputs: labels (B,H,W) i64 (background = n_cls),
 * panoptics (B,H,W) i64 (0 = background, else 1-based rank of the owning box by interior-point
 * count ascending, ties in input order == the reference's stable sort), regression targets
 * (B,8,H,W) f32, points_per_obj (B,H,W) i64, num_objects (1) i32 = boxes owning >= 1 pixel.
 * counts / order / owned: (m) i32 scratch.  No host synchronisation (the reference's loop calls
 * .unique()/.tolist() per sweep, task and instance). */
int rv_assign_targets(const double* cuboids, int32_t m, const int32_t* box_offsets, const float* cart, int32_t B,
                      int32_t H, int32_t W, int32_t n_cls, int32_t azimuth_invariant, int32_t* counts, int32_t* order,
                      int32_t* owned, int64_t* labels, int64_t* panoptics, float* reg_targets,
                      int64_t* points_per_obj, int32_t* num_objects, rvStream stream);

/* Fused detection loss.  logits / regressands are NHWC fp32 with channel strides ld_* (the layout
 * the head kernels write); cart / reg_targets NCHW fp32; mask (B,H,W) u8.
 * forward : sums[24] (f64, device; 16 before round 6) -- [0] sum w*VFL*mask, [1] foreground part, [2] background part,
 *           [3] #foreground, [4..11] un-normalised regression sums per regressand, [12] max(objects,1),
 *           [13] #foreground + smoothing, [15] = 1.0 (the backward pass's device-side factor, below), [16..23] the scalars
 *           detection_head.py:379-449 reports: loss = sums[0]/sums[13] + (sums[4]+...+sums[11])/sums[12], classification, foreground,
 *           background, coordinate, dimension, rotation, regression loss; optional soft targets (B,n_cls,H,W) and foreground map.
 * backward: d loss / d logits, d loss / d regressands (same NHWC strides), scaled by grad_scale * sums[15] -- the caller may copy
 *           the incoming gradient of the loss (a device scalar) into sums[15] instead of multiplying both tensors afterwards;
 *           reads sums[12], sums[13], sums[15] on device (no host round trip).  Padding channels: columns 8 .. ld_reg-1 of d_regressands
 *           are never written.  Columns n_cls .. ld_logits-1 of d_logits are not written either, EXCEPT with ld_logits == 32 (the rows
 *           the head kernels write: eight 16-byte stores per pixel), where the whole row is stored and these columns are all zero.
 *           Padding columns of the inputs are never used: their values cannot reach any output (32-float logits rows are
 *           loaded whole, so they may be read). */
int rv_detection_loss_forward(const float* logits, int32_t ld_logits, const float* regressands, int32_t ld_reg,
                              const float* cart, const uint8_t* mask, const int64_t* labels, const int64_t* panoptics,
                              const float* reg_targets, const int64_t* points_per_obj, const int32_t* num_objects,
                              int32_t B, int32_t n_cls, int32_t H, int32_t W, const float* host_coding_weights,
                              float cls_weight, float reg_weight, float smoothing, float sigma, float alpha, float gamma,
                              int32_t azimuth_invariant, double* sums, float* soft_targets, float* foreground,
                              rvStream stream);
int rv_detection_loss_backward(const float* logits, int32_t ld_logits, const float* regressands, int32_t ld_reg,
                               const float* cart, const uint8_t* mask, const int64_t* labels, const int64_t* panoptics,
                               const float* reg_targets, const int64_t* points_per_obj, const int32_t* num_objects,
                               int32_t B, int32_t n_cls, int32_t H, int32_t W, const float* host_coding_weights,
                               float cls_weight, float reg_weight, float smoothing, float sigma, float alpha, float gamma,
                               int32_t azimuth_invariant, const double* sums, float grad_scale, float* d_logits,
                               float* d_regressands, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Several FPN levels x several tasks (nn/heads/detection_head.py:138-196 forward, :496-665 compute_targets, :202-449 loss +
 * reduce_multiscale_loss).  An ENTRY is one (level, task) pair; entries are ordered level-major (stride-major), tasks in the order of
 * tasks_cfg -- the order of the reference's `losses_list`.  At most RV_ML_MAX_LEVELS levels and RV_ML_MAX_ENTRIES entries.
 * The one-level entry points above keep their signatures and results.
 * ------------------------------------------------------------------------------------- */
#define RV_ML_MAX_LEVELS 8
#define RV_ML_MAX_ENTRIES 16
/* length of one row of loss sums (the layout rv_detection_loss_forward documents) */
#define RV_LOSS_SUMS_LEN 24
int32_t rv_detection_loss_sums_len(void);

typedef struct {
    int32_t stride;    /* the level sees the columns ::stride of the sweep (rows are never strided); W % stride == 0 */
    int32_t use_range; /* fpn_assignment_method == "RANGE" (:568-582): an annotation belongs to the level iff lower < ||centre xyz|| <= upper (fp64) */
    double lower, upper;
} rvTargetLevel;

typedef struct { /* outputs of one entry at the level's resolution Ws = W / stride, every element written */
    int64_t* labels;         /* (B,H,Ws), background = the task's class count */
    int64_t* panoptics;      /* (B,H,Ws), 0 = background, else 1 + rank within (sweep, level, task) */
    float* reg_targets;      /* (B,8,H,Ws), encoded against the strided cart */
    int64_t* points_per_obj; /* (B,H,Ws), the owner's interior-point count AT THE LEVEL'S RESOLUTION */
} rvTargetOut;

/* compute_targets (:496-665) for every level and task in one sequence of launches, no host round trip.  cuboids / box_offsets / cart
 * as rv_assign_targets (full resolution).  The slab tests run ONCE per (full-resolution pixel, box): a hit is added to the counter
 * of every level whose stride divides the pixel's column.  Boxes are ranked per (sweep, level, task) by that STRIDED count (stable,
 * ascending) over the boxes that pass the level's range filter and carry the task's id in the task column (the reference splits by
 * unique(return_counts), i.e. assumes rows sorted by task within a sweep; for such rows the two agree); boxes without a pixel at
 * the level still consume a rank.  task_ids[t] is the value of the task column of task t, task_classes[t] its class count (the
 * background label).  scratch: (3 * n_levels * max(m,1)) i32.  num_objects: (n_levels * n_tasks) i32, entry order, = boxes owning
 * >= 1 pixel of that entry (== the distinct panoptic ids per sweep summed over sweeps, :379-390).  host_* tables are read at call time. */
int rv_assign_targets_multilevel(const double* cuboids, int32_t m, const int32_t* box_offsets, const float* cart, int32_t B,
                                 int32_t H, int32_t W, int32_t n_levels, const rvTargetLevel* host_levels, int32_t n_tasks,
                                 const int32_t* host_task_ids, const int32_t* host_task_classes, int32_t azimuth_invariant,
                                 int32_t* scratch, const rvTargetOut* host_outs, int32_t* num_objects, rvStream stream);

typedef struct { /* one (level, task) of the loss: the tensors rv_detection_loss_forward / _backward take, at the level's resolution */
    const float* logits;
    const float* regressands;
    const float* cart;
    const uint8_t* mask;
    const int64_t* labels;
    const int64_t* panoptics;
    const float* reg_targets;
    const int64_t* points_per_obj;
    const int32_t* num_objects; /* (1) i32 of this entry */
    float* soft_targets;        /* forward, optional */
    float* foreground;          /* forward, optional */
    float* d_logits;            /* backward */
    float* d_regressands;       /* backward */
    int32_t ld_logits, ld_reg, B, n_cls, H, W;
} rvLossEntry;

typedef struct {
    float coding_weights[8];
    float cls_weight, reg_weight, smoothing, sigma, alpha, gamma;
    int32_t azimuth_invariant;
} rvLossParams;

/* DetectionHead.loss + reduce_multiscale_loss (:202-449) over n_entries (level, task) pairs in two phases.
 * sums: (n_entries + 1) rows of RV_LOSS_SUMS_LEN f64 (device).
 * phase one, ONE launch over the entry table (passed by value as a kernel argument: nothing is copied to the device): row e [0..11] as
 *   rv_detection_loss_forward, soft targets and foreground map of every entry;
 * phase two, one small kernel: total_fg = sum_e row e [3] + smoothing and total_objects = max(sum_e num_objects_e, 1) (:379-401); then
 *   per row e [12] = total_objects, [13] = total_fg, [15] = 1, [16..23] the entry's scalars normalised by the two GLOBAL numbers;
 *   row n_entries = each of [16..23] summed over the entries ([16] is the loss), [12] / [13] = n_entries x the global numbers (the
 *   reference sums its collated list, :438-439), [15] = 1 (the backward pass's device-side factor, as sums[15] above).
 * backward, ONE launch: gradients of row n_entries [16] for every entry, scaled by grad_scale * sums[n_entries][15]; reads the
 *   normalisers from the rows on the device.  Padding channels of every entry's gradient buffers as in rv_detection_loss_backward:
 *   d_regressands columns 8 .. ld_reg-1 and d_logits columns n_cls .. ld_logits-1 are not written, except that an entry with
 *   ld_logits == 32 gets its whole d_logits row stored, zeros in the padding columns.  With one entry every tensor and row 0 equal
 *   the one-level entry points' results (the atomically accumulated [0..11] up to the order of the workgroups' additions). */
int rv_detection_loss_multilevel_forward(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                         double* sums, rvStream stream);
int rv_detection_loss_multilevel_backward(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                          const double* sums, float grad_scale, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Soft target assignment with every option of targets_config (math/ops/assignment.py:76-147 compute_classification_targets, :150-161
 * _gaussian, :64-73 iou_2d_axis_aligned): `affinity_fn` GAUSSIAN | BEV, `normalize_affinities`, finite `k`.  With GAUSSIAN, no
 * normalisation and k = inf the affinity is a per-pixel quantity and the loss entry points above compute it themselves; every other
 * combination makes it a per-INSTANCE quantity (a minimum, a k-th largest value).  rv_soft_assign computes it for every entry of a loss
 * table into one fp32 map (B,H,W) per entry -- the final likelihood of every pixel, 0 outside instances and below the instance's
 * threshold -- and the _aff loss pair reads the affinity from the maps; nothing else about the loss changes.
 *
 * An instance is the pixel set `panoptics[b] == p`, p >= 1, of one entry and sweep.  The valid-pixel mask plays no part in the set (a
 * pixel with mask == 0 competes for a top-k slot, as in the reference; the mask enters in the background mask and the loss).
 *   GAUSSIAN: d = ||centre(prediction) - centre(target)||, both decoded like decode_range_view (fp64 rounded to fp32; predictions always
 *             azimuth-invariantly, :112); normalize: d -= min over the instance (:158-159); a = exp(-d / sigma^2).
 *   BEV:      a = clamp(rotated IoU of [x, y, l, w, yaw] of the decoded prediction and target, 0, 1) (:64-73), the geometry of
 *             rv_rotated_iou (bit-exact with the oracle on equal fp32 boxes).  BEV with normalize is an UnboundLocalError in the
 *             reference (:71-72) and an error here.
 *   top k:    k_actual = min(k, |set|) (:129).  TIE RULE (torch.topk leaves it open): a pixel stays iff its affinity is >= the instance's
 *             k_actual-th largest affinity, and != 0 -- a per-instance threshold on the fp32 affinity values, independent of pixel order
 *             and of scheduling; equal to the reference whenever the k-th and (k+1)-th values differ.  A pixel with affinity exactly 0
 *             (BEV: disjoint boxes; GAUSSIAN: underflow) is never foreground, inside the top k or not (:137-140 `likelihoods.bool()`).
 * k: 0 = infinity, else >= 1.  box_offsets (B+1) i32 (device) / m: the CSR of the annotation table that rv_assign_targets* took; a
 * panoptic id of sweep b lies in 1 .. box_offsets[b+1] - box_offsets[b], so n_entries * (m + B) instance slots bound the tables (pixels
 * with an id beyond that are treated as background).  workspace: rv_soft_assign_workspace_bytes (259 u32 per slot: 256 histogram bins,
 * threshold prefix, remaining count, minimum), 16-byte aligned, need not be initialised; may be NULL when k == 0 and normalize == 0.
 * Of each entry regressands / ld_reg, cart, panoptics, reg_targets, B, H, W are read; every element of every map is written.
 * A fixed number of launches whatever the number of instances and sweeps (1 affinity pass, + 1 under normalize, + 9 under finite k: four
 * rounds of an 8-bit radix select on the affinity's bit pattern, then the threshold pass); integer atomics and min only; no host read. */
#define RV_AFFINITY_GAUSSIAN 0
#define RV_AFFINITY_BEV 1
int64_t rv_soft_assign_workspace_bytes(int32_t n_entries, int32_t m, int32_t B);
int rv_soft_assign(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params, int32_t affinity_fn,
                   int32_t normalize, int32_t k, const int32_t* box_offsets, int32_t m, void* workspace,
                   float* const* host_affinity_maps, rvStream stream);
/* rv_detection_loss_multilevel_forward / _backward with the affinity of entry e read from host_affinity_maps[e] (device pointers, host
 * array read at call time) instead of computed per pixel: foreground = (map != 0), soft target = map at the label's class
 * (assignment.py:137-146).  One entry is a legal table: the one-level recipe with a non-default option runs these too. */
int rv_detection_loss_multilevel_forward_aff(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                             const float* const* host_affinity_maps, double* sums, rvStream stream);
int rv_detection_loss_multilevel_backward_aff(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                              const float* const* host_affinity_maps, const double* sums, float grad_scale,
                                              rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Loss kinds: every classification and regression loss the configuration can name (nn/losses/classification.py:14-119,
 * nn/functional/__init__.py:8-49; `_regression_loss` is any of four torch.nn losses).  Per class logit x with soft target t (the fp32
 * value, detached): p = sigmoid(x), sp = softplus(x), bce = sp - x t; alpha / gamma are the rvLossParams fields.
 *   RV_CLS_VARIFOCAL        t > 0 ? t bce : alpha p^gamma bce -- what the entry points above compute.
 *   RV_CLS_FOCAL            alpha_t q^gamma bce with q = p (1 - t) + (1 - p) t and alpha_t = alpha t + (1 - alpha)(1 - t); alpha < 0: no
 *                           alpha_t factor.  Its semantics are DECLARED here: the reference's FocalLoss calls torchvision's
 *                           sigmoid_focal_loss, and torchvision is outside the reference tree (as with rv_wnms); this is the published
 *                           definition, soft t included.  (The reference passes neither alpha nor gamma on, classification.py:83; that
 *                           quirk is the Python class's business, the kernel takes any values.)
 *                           d/dx = alpha_t [gamma q^(gamma-1) p (1-p) (1-2t) bce + q^gamma (p - t)].
 *   RV_CLS_PENALTY_REDUCED  [t == 1] (1-p)^gamma bce + alpha (1-t)^4 p^gamma bce (functional/__init__.py:30-49); the second term runs
 *                           over every element, t == 1 included, where it is 0.
 *                           d/dx = [t == 1] (-(1-p)^gamma (gamma p (sp - x) + (1-p))) + alpha (1-t)^4 p^gamma (gamma (1-p) bce + (p - t)).
 * 1 - p is formed as sigmoid(-x), never by subtraction; gamma 0, 1, 2, 3 are products, any other value goes through powf.
 * Per regressand, on d = r - t, with reg_param = beta (SMOOTH_L1) or delta (HUBER), ignored by the other two:
 *   RV_REG_L1         |d| -- what the entry points above compute
 *   RV_REG_SMOOTH_L1  |d| < beta ? 0.5 d^2 / beta : |d| - 0.5 beta      (beta == 0 is L1, as torch defines it)
 *   RV_REG_HUBER      |d| <= delta ? 0.5 d^2 : delta (|d| - 0.5 delta)
 *   RV_REG_MSE        d^2
 * The element-wise loss and its product with reg_weight are fp32 values, as for L1; the chain 1 / (points_per_obj + smoothing) * mask *
 * coding_weights[j] / 8 is fp64.  Foreground (affinity != 0), background, the normalisers, the sums layout, phase two and
 * grad_scale * sums[n_entries][15] do not depend on the kinds.
 *
 * rv_detection_loss_table_forward / _backward: rv_detection_loss_multilevel_forward / _backward (host_affinity_maps == NULL) and the
 * _aff pair (host_affinity_maps != NULL: one device pointer per entry) with the kinds of *host_kinds.  With kinds {0, 0, any} every
 * tensor equals the existing pairs' bit for bit and the rows up to the order of the atomic additions.  Refused (rv_last_error): NULL
 * kinds, an unknown kind, SMOOTH_L1 with beta < 0, HUBER with delta <= 0, either with a reg_param that is not finite. */
#define RV_CLS_VARIFOCAL 0
#define RV_CLS_FOCAL 1
#define RV_CLS_PENALTY_REDUCED 2
#define RV_REG_L1 0
#define RV_REG_SMOOTH_L1 1
#define RV_REG_HUBER 2
#define RV_REG_MSE 3
typedef struct {
    int32_t cls_kind, reg_kind;
    float reg_param;
} rvLossKinds;
int rv_detection_loss_table_forward(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                    const rvLossKinds* host_kinds, const float* const* host_affinity_maps, double* sums, rvStream stream);
int rv_detection_loss_table_backward(const rvLossEntry* host_entries, int32_t n_entries, const rvLossParams* host_params,
                                     const rvLossKinds* host_kinds, const float* const* host_affinity_maps, const double* sums,
                                     float grad_scale, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Detection evaluation: matching, AP, ATE / ASE / AOE, CDS with the AV2 sensor-dataset metric definitions (csrc/evaluate.hip).
 * The reference calls av2's CPU evaluator (nn/arch/detector.py:457-479); av2 is not part of the reference tree, so -- as for rv_wnms --
 * the semantics are DECLARED here: they restate the published AV2 detection metric and are not pinned against av2's binaries.
 * Pinned to the reference: max_range_m 150 / inf / 55 (datasets/__init__.py:27-39), the detections' range filter on the centre norm
 * (detector.py:573-584), the ground-truth filter num_interior_pts > 0 (prototype/loader.py:583-589) and ASE's IoU
 * prod(min(lwh)) / prod(max(lwh)) (math/ops/iou.py:50-55).
 *
 * Rows are (n,10) f32 [tx_m, ty_m, tz_m, length_m, width_m, height_m, qw, qx, qy, qz]; yaw of a row = 2 atan2(qz, qw), in fp64.
 * Per (sweep, category) segment:
 *   1. evaluated ground truth: gt_valid != 0 (num_interior_pts > 0; NULL = all) and norm2 <= max_range_m^2;
 *   2. evaluated detections: norm2 <= max_range_m^2, in score order, the first `max_num_dts` of them;
 *      norm2 = ((x*x + y*y) + z*z) in fp64 from the fp32 centre, unfused -- every comparison below is on such squares, so that
 *      the flags are bit-reproducible against NumPy;
 *   3. every evaluated detection picks ITS nearest evaluated ground truth (squared centre distance d2 = ((dx*dx + dy*dy) + dz*dz),
 *      fp64 differences of the fp32 centres; ties: the ground truth that comes first in the segment).  A ground truth picked by several
 *      detections goes to the first of them in score order; the others are unmatched (they do not fall through to their second-nearest);
 *   4. tp[t] = matched and d2 <= thresholds_m[t]^2;
 *   5. matched and d2 <= tp_threshold_m^2: err = [ATE = sqrt(d2), ASE = 1 - prod(min(lwh_a, lwh_b)) / prod(max(lwh_a, lwh_b)),
 *      AOE = |yaw_dt - yaw_gt| wrapped to [0, pi]], computed in fp64 and rounded to fp32; NaN otherwise.
 *
 * rv_eval_match -- ONE launch, n_segments + 1 workgroups, asynchronous, no workspace.  The caller orders the rows: dt_order (n_dt) i64
 * lists the detection rows by (segment ascending, score descending, ties in input order), dt_offsets (n_segments + 1) i64 bounds the
 * segments in that list; rows before dt_offsets[0] or from dt_offsets[n_segments] on belong to no segment and are not evaluated.
 * gt_order / gt_offsets: the same for the ground truth, by (segment, input order).  All of them are DEVICE arrays (the grid does not
 * depend on their contents; offsets are clamped to the row counts and an order entry that names no row is skipped).  No bound on the
 * ground truth of a segment (staged through LDS in chunks); max_num_dts <= RV_EVAL_MAX_DTS; n_thresholds <= RV_EVAL_MAX_THRESHOLDS;
 * thresholds_m is a HOST array read at call time.  Outputs in INPUT row order, every element written: dt_evaluated (n_dt) u8,
 * tp (n_dt, n_thresholds) u8, err (n_dt, 3) f32, matched_gt (n_dt) i32 (ground-truth row or -1), gt_evaluated (n_gt) u8.  Claims are
 * resolved with an integer atomicMin in LDS: the result does not depend on scheduling.
 *
 * rv_eval_summarize -- from the rows of all sweeps, ordered by (category ascending, score descending, ties in accumulation order),
 * evaluated rows only in [cat_offsets[c], cat_offsets[c + 1]) (DEVICE, n_categories + 1, i64; rows beyond cat_offsets[n_categories]
 * are ignored), flags (n_rows, n_thresholds) u8 = tp, err (n_rows, 3) f32, n_gt (n_categories) i64 (DEVICE) = evaluated ground truth:
 *   per category and threshold: tp = cumsum(flag), recall = tp / n_gt, precision = tp / (index + 1), made non-increasing from the
 *   right; sampled at linspace(0, 1, num_recall_samples) by linear interpolation as numpy.interp does it (left = precision[0],
 *   right = 0); AP_t = mean of the samples, 0 for a category without evaluated ground truth or detections; AP = mean over t;
 *   ATE / ASE / AOE = mean of the err columns over the rows where they are not NaN, else (tp_threshold_m, default_ase, default_aoe);
 *   CDS = AP * mean(1 - min(ATE / tp_threshold_m, 1), 1 - min(ASE, 1), 1 - min(AOE / pi, 1)).
 * table (n_categories + 1, 5) f64 [AP, ATE, ASE, AOE, CDS], last row = column means over the categories; ap_per_threshold
 * (n_categories, n_thresholds) f64.  fp64 throughout, sums in a fixed order (bit-identical from run to run).  Two launches (one
 * workgroup per (category, threshold); one workgroup for the table), asynchronous.  workspace: rv_eval_summarize_workspace_bytes
 * (12 bytes per row and threshold), 8-byte aligned, need not be initialised.  n_rows < 2^31. */
#define RV_EVAL_MAX_THRESHOLDS 8
#define RV_EVAL_MAX_DTS 1024
int rv_eval_match(const float* dts, const int64_t* dt_order, const int64_t* dt_offsets, int64_t n_dt, const float* gts,
                  const uint8_t* gt_valid, const int64_t* gt_order, const int64_t* gt_offsets, int64_t n_gt, int32_t n_segments,
                  const double* host_thresholds_m, int32_t n_thresholds, double tp_threshold_m, double max_range_m, int32_t max_num_dts,
                  uint8_t* dt_evaluated, uint8_t* tp, float* err, int32_t* matched_gt, uint8_t* gt_evaluated, rvStream stream);
int64_t rv_eval_summarize_workspace_bytes(int64_t n_rows, int32_t n_categories, int32_t n_thresholds);
int rv_eval_summarize(const uint8_t* flags, const float* err, const int64_t* cat_offsets, const int64_t* n_gt, int64_t n_rows,
                      int32_t n_categories, int32_t n_thresholds, double tp_threshold_m, int32_t num_recall_samples, double default_ase,
                      double default_aoe, void* workspace, double* table, double* ap_per_threshold, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * AV2 region of interest (ROI) on the device: the map raster, per-point and per-box flags, the evaluation filter (csrc/roi.hip, and
 * rv_eval_match_roi in csrc/evaluate.hip).  The reference flags every lidar return with av2's map API (converters/av2/export.py:91-97:
 * city_SE3_ego.transform_from, get_raster_layer_points_boolean(ROI)) and evaluates AV2 with eval_only_roi_instances = True
 * (datasets/__init__.py:27-30, nn/arch/detector.py:457-472).  av2 is not part of the reference tree, so -- as for rv_eval_match -- the
 * semantics are DECLARED here and not pinned against av2's binaries.  The free choices, so that a mismatch with av2 can be traced to one
 * of them: (1) raster coordinates are TRUNCATED toward zero to the cell index; (2) a box is inside iff one of its 8 VERTICES is;
 * (3) the matcher applies the per-category CAP BEFORE the ROI flag; (4) the builder fills a pixel by its CENTRE; (5) the dilation keeps
 * offsets with du^2 + dv^2 <= r^2 (`<=`).
 *
 * Atlas: the rasters of any number of logs in ONE u8 device buffer `raster` (raster_bytes long) and a DEVICE table of n_layers rvRoiLayer
 * records: layer k is the row-major (height, width) image at raster + offset, cell (v, u) at offset + v * width + u; (s, tx, ty) is av2's
 * array_Sim2_city with R = I.  rv_roi_atlas_check validates a HOST copy of the table against raster_bytes (every layer inside the
 * buffer, s > 0, finite) before it is uploaded; the kernels additionally never read outside [0, raster_bytes).
 * Sweep table (DEVICE): layer_index (n_sweeps) i32 and city_SE3_ego (n_sweeps, 12) f64, the row-major 3 x 4 [R | t] of each sweep.
 *
 * Lookup of an ego-frame point p = (x, y, z) of sweep b, fp64 from the input type, no fused multiply-add, in this order:
 *   pcx = ((T[0]*x + T[1]*y) + T[2]*z) + T[3];  pcy = ((T[4]*x + T[5]*y) + T[6]*z) + T[7]      (T = city_SE3_ego[b]; z of the city point unused)
 *   a = (pcx + tx) * s;  b = (pcy + ty) * s;  u = (int64)a, v = (int64)b truncating toward zero, as a NumPy integer cast does -- a
 *   coordinate in (-1, 0) therefore lands in cell 0;
 *   flag = raster[v, u] != 0 iff 0 <= u < width and 0 <= v < height, else 0; a non-finite a or b gives 0 (decided as
 *   a > -1 && a < width && b > -1 && b < height, false for NaN, before the cast).
 * A sweep whose layer_index is outside [0, n_layers) gives 0 for all its rows.  A row that belongs to no sweep gets 0 and adds 1 to
 * *stray (DEVICE i64, ACCUMULATED: the caller zeroes it and decides when to read it).
 *
 * rv_roi_points -- xyz (n, 3) f32 or f64 (xyz_is_f64), sweep_offsets (n_sweeps + 1) i64 DEVICE (CSR: sweep b owns the rows
 * [offsets[b], offsets[b + 1]); rows before offsets[0] or from offsets[n_sweeps] on are stray) -> within_roi (n) u8.  One launch, one
 * thread per point (grid-stride), the sweep by binary search.
 * rv_roi_boxes -- boxes (n, 10) f32 [tx_m, ty_m, tz_m, length_m, width_m, height_m, qw, qx, qy, qz], batch_index (n) i64 (outside
 * [0, n_sweeps): stray) -> within_roi (n) u8: 1 iff ANY of the 8 vertices is inside (av2's compute_objects_in_roi_mask looks at vertices
 * only: a box across a thin strip with all vertices outside is out).  Vertices, in fp64 from the fp32 row:
 *   R = [[1 - 2*(qy*qy + qz*qz), 2*(qx*qy - qz*qw), 2*(qx*qz + qy*qw)], [2*(qx*qy + qz*qw), 1 - 2*(qx*qx + qz*qz), 2*(qy*qz - qx*qw)],
 *        [2*(qx*qz - qy*qw), 2*(qy*qz + qx*qw), 1 - 2*(qx*qx + qy*qy)]] -- the full quaternion AS GIVEN (not normalised, not yaw only);
 *   d = (+-0.5*length, +-0.5*width, +-0.5*height);  vertex_i = c_i + ((R[i][0]*d0 + R[i][1]*d1) + R[i][2]*d2), then the lookup above.
 * One launch, one thread per box.
 *
 * rv_roi_rasterize -- builds one layer from drivable-area polygons (the reference ships no builder).  vertices (n_vertices, 2) f64 city
 * frame, polygon_offsets (n_polygons + 1) i64, both DEVICE (offsets clamped to the vertex count); polygon p is the closed ring of its
 * vertices, the last joined to the first.  r = dilation radius in PIXELS (fp64, finite, >= 0).  height * width < 2^31.
 *   1. fill: vertices map to ((x + tx) * s, (y + ty) * s).  Pixel (v, u) is drivable iff its centre (cx, cy) = (u + 0.5, v + 0.5) is
 *      inside ANY polygon by the even-odd rule, where an edge a -> b counts iff (a.y <= cy) != (b.y <= cy) and
 *      a.x + (cy - a.y) * (b.x - a.x) / (b.y - a.y) > cx (fp64, that order).  Vertices are expected to be finite.
 *   2. dilate: a pixel is ROI iff some drivable pixel lies at an integer offset (du, dv) with (double)(du*du + dv*dv) <= r*r; pixels
 *      outside the image are not drivable.  Computed separably (per pixel the horizontal distance to the nearest drivable pixel of its
 *      row, clamped; then dx(dv)^2 + dv^2 over the column), which is the same set.  Integers and booleans only: exact.
 * -> drivable (height, width) u8 and roi (height, width) u8 (r = 0: equal).  Four launches (polygon boxes; fill, one thread per pixel,
 * edges through LDS in chunks, polygons whose box misses the workgroup's tile skipped; rows; columns), asynchronous.  workspace:
 * rv_roi_rasterize_workspace_bytes, 8-byte aligned, need not be initialised.
 *
 * rv_eval_match_roi -- rv_eval_match with the detections' ROI flags dt_roi (n_dt) u8 (NULL: exactly rv_eval_match; both entry points
 * launch one kernel).  Declared order (av2 ANDs the cap mask and the ROI mask): a row IN RANGE counts towards max_num_dts whatever its
 * flag, and evaluated = in range && rank < max_num_dts && dt_roi[row] != 0.  A row with flag 0 gets the outputs of a row that was not
 * evaluated.  For the ground truth the caller ANDs the flag into gt_valid. */
typedef struct rvRoiLayer {
    int64_t offset;
    int32_t height, width;
    double s, tx, ty;
} rvRoiLayer;
int rv_roi_atlas_check(const rvRoiLayer* host_layers, int32_t n_layers, int64_t raster_bytes);
int rv_roi_points(const void* xyz, int32_t xyz_is_f64, int64_t n, const int64_t* sweep_offsets, int32_t n_sweeps,
                  const int32_t* layer_index, const double* city_SE3_ego, const uint8_t* raster, int64_t raster_bytes,
                  const rvRoiLayer* layers, int32_t n_layers, uint8_t* within_roi, int64_t* stray, rvStream stream);
int rv_roi_boxes(const float* boxes, const int64_t* batch_index, int64_t n, int32_t n_sweeps, const int32_t* layer_index,
                 const double* city_SE3_ego, const uint8_t* raster, int64_t raster_bytes, const rvRoiLayer* layers, int32_t n_layers,
                 uint8_t* within_roi, int64_t* stray, rvStream stream);
int64_t rv_roi_rasterize_workspace_bytes(int32_t n_polygons, int32_t height, int32_t width);
int rv_roi_rasterize(const double* vertices, const int64_t* polygon_offsets, int64_t n_vertices, int32_t n_polygons, double s, double tx,
                     double ty, int32_t height, int32_t width, double r, void* workspace, uint8_t* drivable, uint8_t* roi, rvStream stream);
int rv_eval_match_roi(const float* dts, const int64_t* dt_order, const int64_t* dt_offsets, int64_t n_dt, const float* gts,
                      const uint8_t* gt_valid, const int64_t* gt_order, const int64_t* gt_offsets, int64_t n_gt, int32_t n_segments,
                      const double* host_thresholds_m, int32_t n_thresholds, double tp_threshold_m, double max_range_m, int32_t max_num_dts,
                      const uint8_t* dt_roi, uint8_t* dt_evaluated, uint8_t* tp, float* err, int32_t* matched_gt, uint8_t* gt_evaluated,
                      rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Detection evaluation with the Waymo Open Dataset metric definitions: rotated BEV / 3-D IoU, maximum-weight ("Hungarian") matching,
 * AP and APH per object type, range and difficulty level (csrc/evaluate_waymo.hip).  The reference hands its detections to
 * waymo_open_dataset's evaluator (evaluation/evaluate.py:367-466); that library (and TensorFlow) is not part of the reference tree,
 * so -- as for rv_eval_match -- the semantics are DECLARED here and are not pinned against its binaries.  Pinned to the reference: the
 * ground-truth filter and the level rule (evaluate.py:325-333), the object types (:68), frames = the sweeps that have ground truth
 * (:382-389), yaw from the quaternion (:269-286) rounded to fp32 with the box (:407-408), the configuration (:289-319) and the
 * result layout (:70-243).  The declared choices, so that a mismatch with another implementation can be traced to one of them:
 * the weight quantum 1000, the tie rule of the search, matching by prefix insertion, "ignored at this level", the AP integration.
 *
 * Rows are boxes (n,7) f32 [x, y, z, length, width, height, yaw].  A SEGMENT is one (sweep, object type): segment = sweep * 4 + type - 1,
 * type 1 VEHICLE, 2 PEDESTRIAN, 3 SIGN, 4 CYCLIST.  The caller orders the rows as for rv_eval_match: dt_order (n_dt) i64 lists the
 * detections by (segment ascending, score descending, ties in input order), dt_offsets (n_segments + 1) i64 bounds the segments in that
 * list, gt_order / gt_offsets the ground truth by (segment, input order); all DEVICE arrays, offsets clamped to the row counts, an order
 * entry that names no row is skipped, rows outside every segment are not evaluated.  For another order of a segment's detections the
 * result is not defined, but every kernel terminates and stays inside its buffers.
 *
 * IoU of a pair (both fp32, unfused).  BEV: rv_rotated_iou of the rectangles [x - l/2, y - w/2, x + l/2, y + w/2, yaw] (halves formed
 * as 0.5f * l), bit for bit.  3-D: inter = area * max(0, min(za + ha/2, zb + hb/2) - max(za - ha/2, zb - hb/2)) with `area` the
 * intersection area that BEV IoU was formed from, vol = (l * w) * h, iou = inter / (vol_a + vol_b - inter); 0 where a volume or
 * the union is not positive.  A pair whose footprints' circumscribed circles are more than 0.05 % apart is 0 in both without clipping
 * (the clip returns exactly 0 for it as well).
 *
 * Problems.  One per (segment, box type in {BEV, 3-D}, shard in {all ranges, [0,30), [30,50), [50,inf) m}).  A row belongs to a range
 * shard by ITS OWN centre: r2 = ((x*x + y*y) + z*z) in fp64 from the fp32 centre against 900 and 2500, lower bound inclusive -- a
 * detection at 29.9 m on ground truth at 30.1 m is matched in "all ranges" and is a false positive in [0,30).  Ground truth takes part
 * with gt_level != 0 (the caller writes 0 for num_interior_pts <= 0), whatever its level.  Cutoffs: c_k = fp32(k * 0.01), k = 0 .. 99,
 * c_100 = 1; a detection takes part at the cutoffs c_k <= score (fp32 compare; a NaN or negative score at none).
 *
 * Weights.  w(d, g) = min(1000, floor(1000 * iou)) (fp32 product) if iou >= iou_thresholds[type] (fp32 compare), else 0: an integer.
 * A matching maximises the sum of w; a pair of weight 0 is no match.
 *
 * Which optimum, and every cutoff in one pass.  The detections are inserted one at a time in score order, each by ONE shortest-
 * augmenting-path search with potentials on the integer costs -w (Jonker-Volgenant form), with one always-free zero-cost column
 * "unmatched".  Row potentials u and column potentials v start at 0 and are carried from row to row.  Search for row r: every column
 * unused, minv = +inf; i0 = r.  Step: for every unused column j, cur = -w(i0, j) - u[i0] - v[j]; if cur < minv[j], minv[j] = cur and j
 * remembers the column i0 was reached from; "unmatched" likewise keeps dmin = min(dmin, -u[i0]) (strict <: the first row that reached
 * the value).  delta = the least of dmin and the minv of the unused columns: ties go to "unmatched" first, then to the lowest
 * ground-truth position.  u[r] and the u of the owner of every used column grow by delta, v of every used column falls by delta, minv of
 * every unused column and dmin fall by delta.  If "unmatched" won, the search ends there: the row that reached it becomes unmatched
 * (it is never moved again) and every row before it on the path takes the column it was reached from.  Otherwise the winning column
 * becomes used; if it has no owner the path is handed down the same way, else i0 = its owner and the next step follows.  All arithmetic
 * is integer, so the sequential procedure defines the result exactly.  The matching at cutoff c_k is the state after every row with
 * score >= c_k has been inserted: by the invariant of the method it is a maximum-weight matching of exactly those rows, so it differs
 * from a from-scratch solve per cutoff only in WHICH of several equally good assignments is reported.
 * Compaction: a row without any pair of weight > 0 sees cost -v[j] >= 0 = the cost of "unmatched" at every column (v never rises above 0),
 * so its search ends in its first step with delta 0 and changes nothing; a column without such a pair keeps v = 0 and costs -u[i0] from
 * every row, never less than dmin, so with ties going to "unmatched" it is never used.  Neither ever enters a path: the kernel leaves
 * them out of the search (keeping the order of the rest) and counts them directly, with the identical result.
 *
 * Counts per (box type, breakdown row, level L in {1, 2}, cutoff k), summed over the sweeps, int64 [TP, FP, FN, heading]:
 * TP = matched pairs whose ground truth has level <= L; a detection matched to ground truth of level > L is ignored (neither TP nor
 * FP); FP = inserted detections without a match; FN = ground truth of level <= L without a match; heading = sum over the TPs of
 * rint(2^40 * (1 - d / pi)), d = fmod(|yaw_d - yaw_g|, 2 pi) folded to [0, pi] (2 pi - d above pi), fp64 (0 for a NaN).  Every
 * accumulator is an integer: the tables do not depend on how the sweeps are split into calls, on scheduling or on the number of ranks.
 * Breakdown rows: 0 .. 3 the types over all ranges, 4 + 3 (type - 1) + (shard - 1) the type in a range shard.
 *
 * rv_waymo_iou -- the (BEV, 3-D) IoU of every (detection, ground truth) pair of a segment into `workspace`, two launches, asynchronous.
 * Layout: pair_off (n_segments + 1) i64 at byte 0, then, 256-byte aligned, (pairs, 2) f32; the pair (i-th detection, j-th ground truth
 * of segment s, in the orders above) is at pair_off[s] + i * n_gt(s) + j.  A segment beyond a limit has no pairs.  n_segments is any
 * positive number here (the type only enters rv_waymo_match).  workspace: rv_waymo_match_workspace_bytes, 8-byte aligned.
 *
 * rv_waymo_match -- ONE launch, n_sweeps * 32 workgroups (one per problem), asynchronous, on the workspace rv_waymo_iou filled for the same
 * rows (n_segments = 4 * n_sweeps).  scores (n_dt) f32; gt_level (n_gt) u8; sweep_valid (n_sweeps) u8 or NULL: a sweep flagged 0 is no
 * frame (no ground truth left) and none of its rows is counted.  iou_thresholds: 5 HOST floats indexed by type, read at call time.
 * Adds to `tables` (2, 16, 2, 101, 4) i64 (box type, breakdown row, level - 1, cutoff, [TP, FP, FN, heading]; the caller zeroes it once)
 * with 64-bit integer atomics and to `errors` (4) i32: [0] segments with more than RV_WAYMO_MAX_DTS detections, [1] with more than
 * RV_WAYMO_MAX_GTS ground truth (such a segment is not evaluated at all: nothing is truncated), [2] segments whose pair offsets do not
 * fit the workspace, [3] searches that hit their iteration bound (cannot happen; the row stays unmatched).
 *
 * rv_waymo_summarize -- tables -> out (2, 32, 2) f64 (box type, result row, [AP, APH]), one launch.  Result rows: the 4 types x 2 levels
 * over all ranges (type-major), then per type the 3 range shards x 2 levels.  Per row: p_k = TP / (TP + FP), r_k = TP / (TP + FN), 0 when
 * the denominator is 0; for APH both numerators are heading * 2^-40.  Precision is made non-increasing towards higher recall (running
 * maximum from k = 0 upwards), AP = sum over k = 100 .. 0 of (r_k - r_prev) * p_k from r_prev = 0, fp64, in that order. */
#define RV_WAYMO_MAX_DTS 1024
#define RV_WAYMO_MAX_GTS 1024
#define RV_WAYMO_MAX_SWEEPS 65536
#define RV_WAYMO_NUM_CUTOFFS 101
#define RV_WAYMO_NUM_BREAKDOWN_ROWS 16
#define RV_WAYMO_NUM_RESULT_ROWS 32
int64_t rv_waymo_match_workspace_bytes(int64_t n_dt, int64_t n_gt, int32_t n_segments);
int rv_waymo_iou(const float* dts, const int64_t* dt_order, const int64_t* dt_offsets, int64_t n_dt, const float* gts,
                 const int64_t* gt_order, const int64_t* gt_offsets, int64_t n_gt, int32_t n_segments, void* workspace, rvStream stream);
int rv_waymo_match(const float* dts, const float* scores, const int64_t* dt_order, const int64_t* dt_offsets, int64_t n_dt,
                   const float* gts, const uint8_t* gt_level, const int64_t* gt_order, const int64_t* gt_offsets, int64_t n_gt,
                   const uint8_t* sweep_valid, int32_t n_sweeps, const float* host_iou_thresholds, const void* workspace, int64_t* tables,
                   int32_t* errors, rvStream stream);
int rv_waymo_summarize(const int64_t* tables, double* out, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Waymo range image -> sweep: polar (sensor frame, per-pixel pose) to Cartesian (vehicle frame at the frame's timestamp).
 * What the reference's offline exporter (converters/waymo/export.py:55-147 convert_range_image_to_cartesian, :255-285) gets from
 * waymo_open_dataset's range_image_utils.extract_point_cloud_from_range_image, compute_inclination and
 * transform_utils.get_rotation_matrix, for the FIRST return of the TOP lidar (all the reference exports).  DECLARED semantics:
 * neither TensorFlow nor waymo_open_dataset is available to this project, so the rules below restate those functions and are NOT
 * pinned against their binaries (tests/waymo_convert_ref.py is the NumPy restatement the kernels are tested against).
 *
 * Inputs (device pointers, B frames per call):
 *   range_image    (B, H, W, 4) fp32, 16-byte aligned: range, intensity, elongation, nlz.  range <= 0 (or NaN): no return;
 *                  nlz == 1.0: the pixel lies in a no-label zone.
 *   extrinsic      (B, 4, 4) fp64 row-major E: vehicle <- sensor.
 *   inclination    (B, H) fp64: inclination of IMAGE ROW r (row 0 = the highest beam), i.e. the calibration's beam table reversed,
 *                  or, for a uniform sensor, (r + 0.5) / H * (max - min) + min for r = 0 .. H-1, reversed.
 *   pixel_pose     (B, H, W, 6) fp32 or NULL: roll, pitch, yaw, tx, ty, tz of world <- vehicle at the time the pixel was measured.
 *   inv_frame_pose (B, 3, 4) fp64, required iff pixel_pose is given: the upper three rows of V = inverse(world <- vehicle at the
 *                  frame's timestamp), inverted by the caller in fp64.
 * Per pixel (row r, column c), everything in fp64 from the fp32 / fp64 inputs, rounded to fp32 once at the end:
 *   az_correction = atan2(E[1][0], E[0][0]);  ratio = (W - c - 0.5) / W;  azimuth = (2 ratio - 1) pi - az_correction
 *     (column 0 is azimuth ~ +pi);
 *   p_sensor  = range * [cos(azimuth) cos(incl_r), sin(azimuth) cos(incl_r), sin(incl_r)];
 *   p_vehicle = E[:3,:3] p_sensor + E[:3,3];
 *   with a pixel pose: R = Rz(yaw) Ry(pitch) Rx(roll), p_world = R p_vehicle + t, p = V[:3,:3] p_world + V[:3,3]; else p = p_vehicle;
 *   valid = range > 0 and nlz != 1.0.  A valid pixel is [range, intensity, elongation, x, y, z] with the first three bit-equal to
 *   the input; every other pixel is exact +0.0 in all six channels.  This is a SELECT, not the reference's product with a 0/1
 *   mask: a NaN range or pose at an invalid pixel leaves zeros, not NaN (declared deviation).
 *   num_pts[b] (int64, may be NULL; cleared by the call) = number of valid pixels of frame b -- the quantity behind the reference's
 *   `num_pts >= 50000` filter of training frames.
 * fp64 and not TensorFlow's fp32, because the detour through the world frame adds and subtracts kilometres (DESIGN 8.4 has the
 * figures); a table made by the TensorFlow exporter differs from this one by that fp32 error.
 *
 * rv_waymo_range_image_to_sweep: -> sweep (B, H, W, 6) fp32 channel-last, 8-byte aligned: the reference's table, H*W rows of
 *   range, intensity, elongation, x, y, z per frame.
 * rv_waymo_range_image_to_batch: -> the loader's padded batch in the same single launch: features (B, n_feat, H, W + 2 pad) with
 *   feature f = sweep channel host_feat_src[f] (0 .. 5, HOST array, <= 16 entries) through host_feat_op[f] (0 copy, 1 tanh: the
 *   same device function on the same fp32 value as rv_table_to_range_view), cart (B, 3, H, W + 2 pad) = x, y, z,
 *   mask (B, 1, H, W + 2 pad) u8 = valid.  The `pad` columns on either side are zeros, or, with circular != 0, the wrap-around in
 *   azimuth (rv_pad_range_view's rule); num_pts counts the W image columns only.  Equal bit for bit to rv_table_to_range_view +
 *   rv_pad_range_view on the sweep of the first entry.
 * Both: asynchronous on `stream`, own no memory, one kernel launch (plus the clearing of num_pts).  They return non-zero BEFORE
 * anything is launched for: a NULL required pointer, B / H / W <= 0, B or H > 65535 (the launch grid; pixel offsets are 64-bit),
 * pixel_pose without inv_frame_pose or the reverse, a misaligned pointer, n_feat outside 1 .. 16, a feature source outside 0 .. 5,
 * an op other than 0 / 1, pad < 0.
 * ------------------------------------------------------------------------------------- */
int rv_waymo_range_image_to_sweep(const float* range_image, const double* extrinsic, const double* inclination,
                                  const float* pixel_pose, const double* inv_frame_pose, int32_t B, int32_t H, int32_t W, float* sweep,
                                  int64_t* num_pts, rvStream stream);
int rv_waymo_range_image_to_batch(const float* range_image, const double* extrinsic, const double* inclination,
                                  const float* pixel_pose, const double* inv_frame_pose, int32_t B, int32_t H, int32_t W, int32_t n_feat,
                                  const int32_t* host_feat_src, const int32_t* host_feat_op, int32_t pad, int32_t circular,
                                  float* features, float* cart, uint8_t* mask, int64_t* num_pts, rvStream stream);

/* The debug panels of the training loop (rendering/tensorboard.py) and mmcv's IoU ops (csrc/render.hip) are declared, with their full
 * semantics, in include/rv3d_render.h -- a header of its own beside this one, which it includes: this file's list of prototypes, and
 * that of the headers it includes, stay the lists that the binding's census counts.  The binding (`_lib.py`) types its entries
 * exactly as it types this file's.  include/rv3d_optim.h is a second header of that kind: rv_adamw_step for several parameter groups,
 * per-parameter step counts, amsgrad and maximize (rv_adamw_step_groups). */

#ifdef __cplusplus
}
#endif
#endif /* RV3D_H_ */
