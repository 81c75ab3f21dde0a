/*
 * include/mdr_inbatch.h -- C ABI of the in-batch-negative rank step in libmdrhip.so (gfx950).
 *
 * Replaces mhop_eval (mdr/retrieval/criterions.py:153-182) and the forward value of mhop_loss (:114-151) of the
 * reference's scripts/train_mhop.py: for a batch of B questions with embeddings q, q_sp (hop-2 query), c1, c2 (the two
 * gold passages) and two negatives each, row i of a hop is scored against 2B + 2 columns
 *     column j <  B        c1[j]
 *     column B + j         c2[j]          (hop 1: column B + i of row i is -inf, the question's own bridge passage)
 *     columns 2B, 2B + 1   neg[i][0], neg[i][1]
 * and the target is column i (hop 1, rows of q) or B + i (hop 2, rows of q_sp). The [B, 2B + 2] score matrix, the mask
 * and the two argsorts are never formed: one kernel contracts on MFMA, compares every score with the row's target score
 * in the tile epilogue and folds an online log-sum-exp.
 *
 * The conventions of include/mdr_hip.h hold (int return codes, mdr_last_error(), *_dev = device pointers on the current
 * device, `stream` = hipStream_t as void*, caller-owned buffers, everything enqueued on `stream`, no synchronisation).
 *
 * Scores.   mode MDR_INBATCH_F32   fp32 operands, fp32 accumulation (v_mfma_f32_16x16x4_f32): plain torch.mm numerics.
 *           mode MDR_INBATCH_O1    each operand is rounded to fp16 once (round to nearest even), products accumulate in
 *                                  fp32 (v_mfma_f32_16x16x32_f16) and the sum is rounded to fp16: what torch.mm / torch.bmm
 *                                  return under apex O1, the regime of the README's --fp16 runs. Comparisons use those fp16
 *                                  values; the log-sum-exp is taken over them in fp32.
 * Rank.     rank = 1 + #{j : s_j > s_t} + #{j < t : s_j == s_t}, the position a stable descending sort gives the target
 *           (the reference's argsort is not stable: among equal scores its rank is unspecified). The target's own score is
 *           produced by the same tile code as every other column, so it compares equal to itself bit for bit.
 * Non-finite scores.  A NaN score never counts as greater than or equal to anything; a row whose target score is NaN gets
 *           rank 2B + 2 (last). +-inf compare as numbers. The log-sum-exp of a row that holds a NaN is NaN, of a row that
 *           holds +inf is +inf.
 */
#ifndef MDR_INBATCH_H
#define MDR_INBATCH_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_INBATCH_F32 0
#define MDR_INBATCH_O1 1

/* Bytes of device scratch mdr_inbatch_rank needs for this shape (0 for an unsupported shape; may be 0 for a supported one:
 * the partial results of a row tile live in LDS). */
size_t mdr_inbatch_workspace_bytes(int B, int d, int mode);

/* q_dev, qsp_dev fp32 [B, d]; ctx_dev fp32 [2B, d] = the rows of c1, then the rows of c2; neg_dev fp32 [B, 2, d].
 * B >= 1; d a multiple of 32 with 32 <= d <= 1024. rank1_dev / rank2_dev int32 [B], 1-based (required).
 * tscore*_dev fp32 [B]: the target score as it was compared (mode O1: the fp16 value widened); lse*_dev fp32 [B]: the
 * log-sum-exp over the row's 2B + 2 scores, the -inf column excluded, so that mhop_loss = mean(lse1 - tscore1) +
 * mean(lse2 - tscore2). Those four may be NULL. workspace_dev may be NULL when mdr_inbatch_workspace_bytes is 0. */
int mdr_inbatch_rank(const float* q_dev, const float* qsp_dev, const float* ctx_dev, const float* neg_dev, int B, int d, int mode,
                     int32_t* rank1_dev, int32_t* rank2_dev, float* tscore1_dev, float* tscore2_dev, float* lse1_dev, float* lse2_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

/* the in-batch loss with the memory bank and its gradients: same conventions, same modes, its own header */
#include "mdr_inbatch_loss.h"

#endif /* MDR_INBATCH_H */
