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

#ifdef __cplusplus
}
#endif
#endif /* RV3D_OPTIM_H_ */
