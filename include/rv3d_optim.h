/* rv3d_optim.h -- the optimiser step with torch.optim.AdamW's parameter-group semantics (csrc/optim.hip): a companion of rv3d.h, which
 * it includes (rvStream, the error contract: an int-returning entry returns non-zero and rv_last_error() says why).  A C / C++ caller
 * includes this file; the Python binding (`_lib.py`, `optim_prototypes()`) types its entries exactly as it types rv3d.h's. */
#ifndef RV3D_OPTIM_H_
#define RV3D_OPTIM_H_
#include "rv3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * rv_adamw_step (rv3d.h) for SEVERAL parameter groups, per-parameter step counts, amsgrad and maximize -- everything
 * torch.optim.AdamW.step() does with its param_groups (torch/optim/adam.py: Adam._init_group collects, per group, the parameters
 * that have a gradient; _multi_tensor_adam bias-corrects every parameter with ITS OWN state["step"]) -- still in two launches for all
 * parameters of all groups, with ONE clipping norm over all of them (torch.nn.utils.clip_grad_norm_ over every parameter, which is what
 * Lightning's gradient_clip_val does).
 *
 * tensors / chunks / partial: as rv_adamw_step, one table over all groups.  tensor_row: n_tensors int32 on the DEVICE, the row of
 * `rows` each tensor is updated with.  vmax: n_tensors DEVICE pointers on the device, max_exp_avg_sq of the tensors whose row carries
 * RV_ADAM_AMSGRAD and NULL for the others; the argument itself may be NULL when no row carries the flag.
 * rows: a HOST array of n_rows rvAdamRow, one per distinct (parameter group, step count) present in this step; 1 <= n_rows <=
 * rv_adam_max_rows().  `step` is the 1-based count of the bias corrections.  The library forms the fp32 scalars of every row exactly
 * as rv_adamw_step forms them (in double, each rounded once: 1 - lr wd, 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^step),
 * sqrt(1 - beta2^step), eps) and passes them to the kernel BY VALUE in its arguments: no upload, no third launch.
 *
 * Launch 1 is rv_adamw_step's sum of squares (the norm depends neither on the groups nor on the sign).  max_norm > 0: every gradient
 * of every group is scaled by the one coefficient min(1, max_norm / (||g||_2 + 1e-6)) on the fly; the stored gradients stay untouched;
 * total_norm (optional) receives ||g||_2, summed in rv_adamw_step's fixed order.
 * Launch 2, per element in fp32, operation by operation as _multi_tensor_adam with decoupled_weight_decay:
 *   RV_ADAM_MAXIMIZE:  g = -g                                  (_foreach_neg, first)
 *   p *= 1 - lr wd;  m = m + (g - m)(1 - beta1);  v = v beta2 + g g (1 - beta2)
 *   RV_ADAM_AMSGRAD:   vmax = max(vmax, v) (_foreach_maximum_), and vmax stands for v below
 *   p -= (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * A row without flags is rv_adamw_step's expression (the same device function).
 * Returns non-zero before anything is launched for a null required argument, n_rows outside 1 .. rv_adam_max_rows(), a row with
 * step < 1 or a beta outside [0, 1), or a row with RV_ADAM_AMSGRAD while vmax is NULL.  A tensor whose tensor_row is outside
 * 0 .. n_rows - 1 is left untouched by the kernel; the caller checks the column when it builds it.
 * Replaces, per group and per distinct step count, ATen's foreach neg / mul / lerp / addcmul / maximum / sqrt / div / add / addcdiv
 * launches, and clip_grad_norm_'s foreach norm, stack, norm, clamp and foreach mul.
 * ------------------------------------------------------------------------------------- */
#define RV_ADAM_AMSGRAD 1
#define RV_ADAM_MAXIMIZE 2
typedef struct rvAdamRow {
    double lr, beta1, beta2, eps, weight_decay;
    int64_t step;
    int32_t flags;
} rvAdamRow;
int32_t rv_adam_max_rows(void);
int rv_adamw_step_groups(const void* tensors, const int32_t* tensor_row, const void* vmax, const void* chunks, int32_t n_chunks,
                         float* partial, const rvAdamRow* rows, int32_t n_rows, double max_norm, float* total_norm, rvStream stream);

/* ---------------------------------------------------------------------------------------
 * Weight averaging -- torch.optim.swa_utils.AveragedModel: the exponential moving average (get_ema_multi_avg_fn) or the equal average
 * (get_swa_multi_avg_fn) of the weights, both one torch._foreach_lerp_(averaged, current, weight) per update -- inside the optimiser's
 * second launch, where every updated parameter is in registers, and as one launch for the tensors the optimiser did not step.
 *
 * rv_adamw_step_groups_avg is rv_adamw_step_groups plus two arguments.  avg: n_tensors DEVICE pointers on the device, the averaged
 * twin of each tensor (fp32, as many elements as the parameter), NULL for a tensor that is not averaged (the idea of `vmax`); the
 * argument itself is required.  avg_weight: ONE weight for all tensors, in [0, 1], rounded to fp32 once on the host (w).
 * Launch 1 is unchanged.  Launch 2 does, after the Adam update of an element and with the new p still in registers,
 *   a = w < 0.5 ? a + w (p - a) : p - (p - a)(1 - w)           (at::lerp's expression, in fp32; w == 1 stores p exactly)
 * The parameters and moments come out bit for bit as from rv_adamw_step_groups on the same inputs (the same element functions); the
 * amsgrad / maximize / clipping / row semantics are its own.  The 16-byte path of a chunk needs `a` aligned like p, g, m and v; a chunk
 * with a misaligned `a` takes the scalar path.  Added traffic: 8 B per averaged element (a read and written once), nothing else.
 * Returns non-zero before anything is launched for what rv_adamw_step_groups refuses, a NULL avg, or avg_weight outside [0, 1] (NaN
 * included).
 * Replaces AveragedModel.update_parameters' foreach lerp over the stepped parameters (12 B per element: a, p in, a out) behind the step.
 *
 * rv_average_tensors is the same expression as ONE multi-tensor launch over fp32 tensors the step did not cover: parameters without a
 * gradient, BatchNorm's running_mean / running_var under use_buffers=True, and -- avg_weight = 1 -- the plain copy of the buffers under
 * use_buffers=False.  table: n_tensors rows (avg, src, n) on the DEVICE: two device pointers and an int64 element count (24 B).
 * chunks: n_chunks int32 pairs (tensor, chunk) on the device, chunk = a run of rv_optim_chunk_elems() elements, as rv_adamw_step's;
 * one workgroup per chunk.  avg and src of a row may be the same address or disjoint, nothing in between.
 * Returns non-zero before anything is launched for a NULL table or chunks, n_chunks <= 0, or avg_weight outside [0, 1].  The rows are
 * on the device, so the host cannot read them: a row with a NULL pointer, or a chunk that starts at or beyond the row's n, is left
 * untouched by the kernel; the caller checks the table when it builds it.
 * Replaces one foreach lerp (or one copy_ per buffer: ~234 launches on the 78 BatchNorm layers of the rv-av2 model) per update.
 * ------------------------------------------------------------------------------------- */
int rv_adamw_step_groups_avg(const void* tensors, const int32_t* tensor_row, const void* vmax, const void* avg, double avg_weight,
                             const void* chunks, int32_t n_chunks, float* partial, const rvAdamRow* rows, int32_t n_rows, double max_norm,
                             float* total_norm, rvStream stream);
int rv_average_tensors(const void* table, const void* chunks, int32_t n_chunks, double avg_weight, rvStream stream);

#ifdef __cplusplus
}
#endif
#endif /* RV3D_OPTIM_H_ */
