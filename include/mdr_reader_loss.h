/*
 * include/mdr_reader_loss.h -- C ABI of the answer reader's training loss and of its three heads with gradients in libmdrhip.so (gfx950):
 * the training branch of the reference's QAModel.forward (mdr/qa/qa_model.py:73-102) and what lies between it and the trunk's last hidden
 * states. The conventions of include/mdr_hip.h hold (int return codes, mdr_last_error(), *_dev = device pointers, `stream` = hipStream_t
 * as void*, caller-owned buffers, everything enqueued on `stream`, no synchronisation). fp16 tensors are passed as their bit patterns.
 *
 * The loss. Inputs: start / end logits fp16 [B, L] (-inf outside the paragraph mask and on padding: what mdr_reader_forward and
 * mdr_reader_heads_forward write), rank fp16 [B], sp fp16 [B, NS] or NULL, starts / ends int64 [B, A] (-1 = ignore), label int64 [B],
 * sent_offsets / sent_labels int64 [B, NS]. All arithmetic is fp32 on the widened fp16 values (CrossEntropyLoss and the BCEs run in fp32
 * under apex O1). Per row b and candidate a
 *     ls = lse_s - start[s_a] if s_a != -1, else 0;   le likewise;   log_prob = -(ls + le)
 * with the log-sum-exp over the entries that are not -inf. A candidate is masked iff log_prob == 0 exactly (both sides ignored, or an
 * fp32 loss of exactly 0); a one-sided candidate counts with its valid side. M_b = sum of exp(log_prob) over the unmasked candidates; the
 * row counts iff M_b != 0;   span_loss = -sum over counted rows of log M_b   (0 with no counted row).
 *     rank_loss = sum_b bce_with_logits(rank_b, label_b)
 *     sp_loss   = sum_bj bce_with_logits(sp_bj, sent_labels_bj) * float(sent_offsets_bj) * float(label_b)      (the offset's VALUE, :78)
 *     loss      = rank_loss + span_loss + sp_weight * sp_loss                                       (the last term absent when sp is NULL)
 * A position outside [0, L) other than -1 is the caller's error; it is treated as -1 and never read.
 *
 * The backward reads the upstream gradient g0 from device memory. With w_a = exp(log_prob_a) / M_b (unmasked candidates of counted rows)
 *     d_start[b, l] = g0 * sum_{a: s_a != -1} w_a (softmax_s[b, l] - [l = s_a]),   d_end likewise,   0 at -inf logits and in uncounted rows
 *     d_rank[b]     = g0 (sigmoid(rank_b) - label_b)
 *     d_sp[b, j]    = g0 * sp_weight * offset_bj * label_b * (sigmoid(sp_bj) - sent_labels_bj)
 * each computed in fp32 and rounded to fp16 once (beyond the fp16 range: infinity of the value's sign). Non-finite inputs propagate by
 * IEEE rules: a row whose logits are all -inf gives a NaN loss, and nothing faults.
 *
 * The heads. h16 fp16 [T, H] packed rows with cu int32 [B + 1] (row b's token p is packed row cu[b] + p), dense16 fp16 [B, H] the pooler
 * dense output, w_head16 fp16 [4, H] the rows start, end, rank, sp and b_head fp32 [4] their biases (already rounded to fp16 values, as apex
 * O1 casts them). mdr_reader_heads_forward launches the kernels of mdr_reader_forward on these tensors: given the same h16 and dense16
 * its bits are the inference forward's. The backward takes fp16 gradients of the four score tensors and writes
 *     d_h16 [T, H]      fp16( g_s[t] W[0] + g_e[t] W[1] + sum_{j: cu[b] + off_bj = t} g_sp[b, j] W[3] ), fp32 terms, one rounding; rows below
 *                       cu[B] in full (0 where no head reads them), rows at or behind cu[B] not at all
 *     d_dense16 [B, H]  fp16( fp16(g_rank[b] W[2, e]) * (1 - pooled16^2) ),  pooled16 = fp16(tanh(dense16))
 *     dw_qa [2, H], db_qa [2], dw_sp [H], db_sp [1], dw_rank [H], db_rank [1]   fp32; with accumulate != 0 added to what the buffers hold,
 *                       the old value last
 * Gradients at positions the forward masked (paragraph_mask != 1, p >= len, an offset outside the row) are taken as 0 whatever the
 * buffers hold there.
 *
 * No atomics anywhere: every output element has one owner and one summation order, which is a function of the shapes alone, so two runs
 * give the same bits.
 *
 * Limits: B >= 1, 1 <= L <= 512 (loss), A >= 1, NS >= 0, H a multiple of 128 in 128 .. 1024, B * L < 2^31; the [.., H] tensors and the
 * workspaces 16-byte aligned (the score tensors, their gradients and the [1] / [2] bias gradients need their element's alignment only).
 * What the host can see is validated: MDR_E_INVALID or MDR_E_WORKSPACE with mdr_last_error() and without a launch.
 */
#ifndef MDR_READER_LOSS_H
#define MDR_READER_LOSS_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device scratch of mdr_reader_loss_forward: the rows' partial losses [3][B]. 0 for a shape outside the limits. */
size_t mdr_reader_loss_workspace_bytes(int batch, int seq_len, int n_cand, int n_sent);

int mdr_reader_loss_forward(const uint16_t* start_logits_dev, const uint16_t* end_logits_dev, const uint16_t* rank_score_dev,
                            const uint16_t* sp_score_dev, const int64_t* starts_dev, const int64_t* ends_dev, const int64_t* label_dev,
                            const int64_t* sent_offsets_dev, const int64_t* sent_labels_dev, int batch, int seq_len, int n_cand, int n_sent,
                            float sp_weight, float* loss_dev, void* workspace_dev, size_t workspace_bytes, int device, void* stream);

int mdr_reader_loss_backward(const uint16_t* start_logits_dev, const uint16_t* end_logits_dev, const uint16_t* rank_score_dev,
                             const uint16_t* sp_score_dev, const int64_t* starts_dev, const int64_t* ends_dev, const int64_t* label_dev,
                             const int64_t* sent_offsets_dev, const int64_t* sent_labels_dev, int batch, int seq_len, int n_cand, int n_sent,
                             float sp_weight, const float* g0_dev, uint16_t* d_start_dev, uint16_t* d_end_dev, uint16_t* d_rank_dev,
                             uint16_t* d_sp_dev, int device, void* stream);

/* sp_score_dev may be NULL (or n_sent 0): no sp head. The other three outputs are required. */
int mdr_reader_heads_forward(const void* h16_dev, const int* cu_dev, const void* dense16_dev, const int64_t* paragraph_mask_dev,
                             const int64_t* sent_offsets_dev, int batch, int seq_len, int n_sent, int hidden, const void* w_head16_dev,
                             const float* b_head_dev, uint16_t* start_logits_dev, uint16_t* end_logits_dev, uint16_t* rank_score_dev,
                             uint16_t* sp_score_dev, int device, void* stream);

/* Bytes of device scratch of mdr_reader_heads_backward: the token chunks' partial sums of dw_qa and dw_sp. 0 outside the limits. */
size_t mdr_reader_heads_backward_workspace_bytes(int batch, int seq_len, int hidden);

/* rows_cap: the rows of h16 and d_h16 (no row at or behind it is touched, whatever cu says). g_sp, dw_sp and db_sp may be NULL together. */
int mdr_reader_heads_backward(const void* h16_dev, const int* cu_dev, const void* dense16_dev, const int64_t* paragraph_mask_dev,
                              const int64_t* sent_offsets_dev, int batch, int seq_len, int n_sent, int hidden, int rows_cap,
                              const void* w_head16_dev, const uint16_t* g_start_dev, const uint16_t* g_end_dev, const uint16_t* g_rank_dev,
                              const uint16_t* g_sp_dev, void* d_h16_dev, void* d_dense16_dev, float* dw_qa_dev, float* db_qa_dev,
                              float* dw_sp_dev, float* db_sp_dev, float* dw_rank_dev, float* db_rank_dev, int accumulate, void* workspace_dev,
                              size_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_READER_LOSS_H */
