/*
 * include/mdr_optim_adamw.h -- the optimizer step of include/mdr_optim.h with the weight decay's form as an argument. Everything of that
 * header holds (table, chunks, state, the norm and finalize kernels, the skip on a non-finite gradient, zero_grads); only the update (c)
 * has a second form.
 *
 * decay_mode = MDR_OPTIM_DECAY_L2 (0): torch.optim.Adam. mdr_optim_step IS this call; same bits.
 * decay_mode = MDR_OPTIM_DECAY_DECOUPLED (1): transformers.AdamW of the reference's era with correct_bias=True, what its
 *     scripts/train_qa.py trains the reader with -- written down as remembered, not captured: no copy of that class is at hand. Per element
 *     of every tensor with a g, unless the step is skipped:
 *         gh = g * mult                                        (no decay in gh)
 *         m  = beta1 * m + (1 - beta1) * gh                    v = beta2 * v + ((1 - beta2) * gh) * gh
 *         denom = sqrt(v) + eps                                step = (lr * sqrt(bias2)) / bias1        (once per launch)
 *         p  = p - step * (m / denom)
 *         p  = p - (lr * weight_decay) * p                     (only where weight_decay != 0; the UPDATED p enters)
 *         p16 = fp16(p)
 *     each operation one correctly rounded fp32 operation, none contracted (csrc/mdr_optim.hip, rounding point 5w, lists them in order).
 *     It differs from mode 0 in three places: the decay never reaches m and v, eps is added outside the bias correction, and the decay is
 *     a shrink of p by lr * weight_decay after the Adam step.
 * Any other decay_mode: MDR_E_INVALID without a launch.
 */
#ifndef MDR_OPTIM_ADAMW_H
#define MDR_OPTIM_ADAMW_H

#include "mdr_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_OPTIM_DECAY_L2 0
#define MDR_OPTIM_DECAY_DECOUPLED 1

int mdr_optim_step_ex(const void* table_dev, int n_tensors, int n_chunks, mdr_optim_state* state_dev, float lr, float beta1, float beta2, float eps,
                      float max_grad_norm, int dynamic, int scale_window, float max_scale, int zero_grads, int decay_mode, void* workspace_dev,
                      size_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_OPTIM_ADAMW_H */
