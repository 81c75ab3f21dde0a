/*
 * include/mdr_optim.h -- C ABI of the optimizer step in libmdrhip.so (gfx950): unscaling by the dynamic loss scale, the global-norm clip
 * and torch.optim.Adam (L2 decay into the gradient, not AdamW) over a table of parameter tensors, and the momentum encoder's EMA over two
 * such tables. The conventions of include/mdr_hip.h hold (int return codes, mdr_last_error(), *_dev = device pointers, `stream` =
 * hipStream_t as void*, caller-owned buffers, everything enqueued on `stream`, no synchronisation and no host readback anywhere).
 *
 * The tensor table. One mdr_optim_tensor per parameter tensor: p, g, m, v fp32 and 16-byte aligned, p16 fp16 (8-byte aligned) or NULL,
 * n >= 1 elements (any value), weight_decay. A descriptor whose g is NULL takes no part in a step: its p, m, v and p16 are neither read nor
 * written, it gets no decay and adds nothing to the norm (torch's Adam on a parameter without .grad).
 *
 * Chunks. The elements are cut into chunks of MDR_OPTIM_CHUNK elements; tensor i owns ceil(n_i / MDR_OPTIM_CHUNK) consecutive chunks, the
 * last one short, so every chunk lies inside one tensor. The split is a function of the n's alone (mdr_optim_chunks). The device table is
 * one blob, written on the host by mdr_optim_table_fill and uploaded by the caller: the n_tensors descriptors, then one (tensor, chunk
 * within the tensor) pair of ints per chunk.
 *
 * mdr_optim_step enqueues three kernels (csrc/mdr_optim.hip lists the rounding points):
 *   (a) norm:     per chunk, the fp32 sum of (g * (1 / loss_scale))^2 and the flag "some g is not finite", into the chunk's own workspace
 *                 slot. A chunk's bits depend on that chunk's gradients only.
 *   (b) finalize: one workgroup adds the chunk sums in a fixed order in fp64;
 *                     grad_norm = fp32(sqrt(sum))   clip_coef = min(1, max_grad_norm / (grad_norm + 1e-6f))   mult = clip_coef / loss_scale
 *                 and moves the state. A flag set, or a sum that is not finite: skipped_last = 1, skipped_total += 1, with dynamic
 *                 loss_scale /= 2 and unskipped = 0; adam_step, b1_pow, b2_pow stay. Otherwise: skipped_last = 0, adam_step += 1,
 *                 b1_pow *= beta1, b2_pow *= beta2, bias += (1 - bias) * (1 - beta) for bias1 and bias2, unskipped += 1, and with dynamic,
 *                 when unskipped == scale_window, loss_scale = min(max_scale, 2 * loss_scale) and unskipped = 0. (apex's dynamic
 *                 LossScaler: 2^16, 2000, 2^24.) bias1 = 1 - beta1^adam_step and bias2 = 1 - beta2^adam_step are Adam's bias corrections,
 *                 carried in this form because 1 - fp32(beta2^k) cancels: b2_pow is within 2^-25 of its value, which is 3e-5 of
 *                 1 - 0.999^k at k = 1 and put the step 1e-5 off torch's. b1_pow and b2_pow are kept for the record only.
 *   (c) update:   per element of every tensor with a g, unless the step is skipped (then p, m, v, p16 keep their bits):
 *                     gh = g * mult                     gd = gh + weight_decay * p   (only where weight_decay != 0)
 *                     m  = beta1 * m + (1 - beta1) * gd  v  = beta2 * v + ((1 - beta2) * gd) * gd
 *                     p  = p - (lr / bias1) * (m / (sqrt(v) / sqrt(bias2) + eps))
 *                 each operation one correctly rounded fp32 operation, none contracted. p16 = fp16(p), round to nearest even, where given.
 *                 With zero_grads, g becomes +0 whether the step is skipped or not.
 * mdr_optim_ema: k = k * fp32(m) + q * fp32(1 - m) (two multiplies and an add, not contracted) and p16 = fp16(k) where table_k gives one.
 *
 * include/mdr_optim_adamw.h declares mdr_optim_step_ex, this step with the decay's form as an argument: mode 0 is mdr_optim_step, mode 1
 * is AdamW (decoupled decay, eps outside the bias correction), which the answer reader trains with.
 *
 * No atomics: two runs from the same inputs give the same bits in p, m, v, p16 and the state.
 *
 * Validated on the host without a launch, MDR_E_INVALID with mdr_last_error(): a NULL table, state or sizes, a negative or zero size, a
 * chunk count that is not the sizes', a misaligned pointer, betas outside [0, 1), eps <= 0 or not finite, scale_window < 1, a flag that is
 * neither 0 nor 1. MDR_E_WORKSPACE: a short or missing workspace. What lies behind the device pointers is the caller's to keep right.
 */
#ifndef MDR_OPTIM_H
#define MDR_OPTIM_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_OPTIM_CHUNK 4096 /* elements of a chunk */

typedef struct mdr_optim_tensor {
    float* p;           /* the fp32 master */
    float* g;           /* its gradient, or NULL: the tensor takes no part in a step */
    float* m;           /* Adam's first moment */
    float* v;           /* Adam's second moment */
    void* p16;          /* fp16 copy of p, or NULL */
    int64_t n;          /* elements, >= 1 */
    float weight_decay; /* L2 decay added to the gradient after the clip; 0 = none */
    int reserved0;
    int64_t reserved1; /* (64 bytes) */
} mdr_optim_tensor;

typedef struct mdr_optim_state {
    float loss_scale;
    int unskipped;     /* clean steps since the scale last moved */
    int adam_step;     /* steps that updated the parameters */
    float b1_pow;      /* beta1 ^ adam_step, one fp32 multiply per step */
    float b2_pow;      /* beta2 ^ adam_step */
    int skipped_last;  /* 1 when the last step found a non-finite gradient */
    float grad_norm;   /* of the last step, unscaled */
    float clip_coef;
    float mult;        /* clip_coef / loss_scale: what the last update multiplied g by */
    int skipped_total;
    float bias1;       /* 1 - beta1 ^ adam_step, by bias += (1 - bias) * (1 - beta1): no cancellation */
    float bias2;       /* 1 - beta2 ^ adam_step */
} mdr_optim_state;

/* The split: the number of chunks of tensors of sizes n[0 .. n_tensors), a function of the sizes ONLY. first_chunk (may be NULL) gets
 * n_tensors + 1 entries: tensor i owns chunks first_chunk[i] .. first_chunk[i + 1]. -1 for a NULL n, n_tensors < 1, a size < 1 or more than
 * 2^31 - 1 chunks. */
int64_t mdr_optim_chunks(const int64_t* n, int n_tensors, int64_t* first_chunk);

/* Bytes of the device table (descriptors + chunk map) and of the workspace (one 8-byte slot per chunk), each a multiple of 256. 0 for
 * sizes mdr_optim_chunks refuses. */
size_t mdr_optim_table_bytes(const int64_t* n, int n_tensors);
size_t mdr_optim_workspace_bytes(const int64_t* n, int n_tensors);

/* Writes the table of `tensors` into table_host (table_bytes >= mdr_optim_table_bytes of their sizes); the caller uploads it. Returns the
 * number of chunks through *n_chunks. */
int mdr_optim_table_fill(const mdr_optim_tensor* tensors, int n_tensors, void* table_host, size_t table_bytes, int* n_chunks);

/* Enqueues the initial state: loss_scale as given (> 0, finite), b1_pow = b2_pow = 1, everything else 0 (bias1 = bias2 = 0). */
int mdr_optim_state_init(mdr_optim_state* state_dev, float loss_scale, int device, void* stream);

int mdr_optim_step(const void* table_dev, int n_tensors, int n_chunks, mdr_optim_state* state_dev, float lr, float beta1, float beta2, float eps,
                   float max_grad_norm, int dynamic, int scale_window, float max_scale, int zero_grads, void* workspace_dev,
                   size_t workspace_bytes, int device, void* stream);

/* table_k and table_q are tables of the same sizes (same n_tensors and n_chunks); only p, p16 and n of the descriptors are used, and a tensor
 * is swept over the smaller of its two n's. */
int mdr_optim_ema(const void* table_k_dev, const void* table_q_dev, int n_tensors, int n_chunks, double m, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_OPTIM_H */
