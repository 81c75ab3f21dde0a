/*
 * include/mdr_inbatch_loss.h -- C ABI of the in-batch retrieval loss with the memory bank, and of its gradients, in libmdrhip.so
 * (gfx950): mhop_loss (mdr/retrieval/criterions.py:114-151 of the reference) with its --momentum branch. include/mdr_inbatch.h ends
 * by including this file; the conventions, the column layout, the mask, the targets and the two score modes are those stated there.
 *
 * Columns 2B + 2 ... 2B + 1 + K of every row are the K rows of queue_dev (fp32 [K, d]; NULL iff K == 0): the same for every
 * row, never masked, never a target, and never written (the reference detaches the queue). Per hop h and row i, with scores s_ij:
 *     lse_i = fp32 log-sum-exp over the unmasked columns          loss = mean(lse1 - tscore1) + mean(lse2 - tscore2)
 *     p_ij  = exp(s_ij - lse_i), 0 at the masked column           g_ij = (p_ij - [j = t_i]) * g0 / B
 *     dq_i = sum_j g1_ij col_j      dqsp_i = sum_j g2_ij col_j    (context, own negatives and queue)
 *     dctx_j = sum_i g1_ij q_i + g2_ij qsp_i                      dneg_i,m = g1_i,(2B+m) q_i + g2_i,(2B+m) qsp_i
 * g0 is the upstream gradient (an amp loss scale enters here), read from DEVICE memory so that the host never synchronises.
 * Mode O1 on the way back (apex O1 as remembered, not captured): g is rounded to fp16 once; the backward of each mm / bmm call
 * contracts fp16 g with the fp16-rounded operand in fp32, rounds the sum to fp16 and widens it; the terms of one leaf (context,
 * queue and negatives terms of dq; the two hops' terms of dctx and dneg) are added in fp32.
 * No atomics: every output element has one owner and one summation order, two runs give the same bits. With K == 0 the forward's
 * lse and tscore equal mdr_inbatch_rank's bit for bit. Non-finite inputs propagate by IEEE rules alone: a row whose lse is NaN
 * has NaN gradients in its own dq / dqsp / dneg rows and in every dctx row it contributes to; nothing faults.
 * B >= 1; d a multiple of 32 with 32 <= d <= 1024; 0 <= K <= 2^26.
 */
#ifndef MDR_INBATCH_LOSS_H
#define MDR_INBATCH_LOSS_H

#include "mdr_inbatch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device scratch that serve both calls below for this shape (0 for an unsupported shape). */
size_t mdr_inbatch_loss_workspace_bytes(int B, int d, int64_t K, int mode);

/* Inputs as mdr_inbatch_rank. tscore*_dev, lse*_dev fp32 [B], all required. */
int mdr_inbatch_loss_forward(const float* q_dev, const float* qsp_dev, const float* ctx_dev, const float* neg_dev, const float* queue_dev, int64_t K,
                             int B, int d, int mode, float* tscore1_dev, float* tscore2_dev, float* lse1_dev, float* lse2_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream);

/* lse*_dev: what the forward wrote for the same inputs. g0_dev: one fp32 on the device. dq_dev, dqsp_dev fp32 [B, d]; dctx_dev fp32
 * [2B, d] (the rows of dc1, then of dc2); dneg_dev fp32 [B, 2, d]; all written in full, 16-byte aligned. */
int mdr_inbatch_loss_backward(const float* q_dev, const float* qsp_dev, const float* ctx_dev, const float* neg_dev, const float* queue_dev, int64_t K,
                              int B, int d, int mode, const float* lse1_dev, const float* lse2_dev, const float* g0_dev, float* dq_dev, float* dqsp_dev,
                              float* dctx_dev, float* dneg_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_INBATCH_LOSS_H */
