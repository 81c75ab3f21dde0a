/*
 * include/mdr_attention_grad.h -- C ABI of the backward of self-attention on packed, ragged rows in libmdrhip.so (gfx950): the gradient of
 * the context the trunk's attention kernels compute (mdr_test_attention of include/mdr_hip.h) with respect to Q, K and V. The conventions
 * of include/mdr_hip.h hold (int return codes, mdr_last_error(), *_dev = device pointers, `stream` = hipStream_t as void*, caller-owned
 * buffers, everything enqueued on `stream`, no synchronisation).
 *
 * Layout. qkv_dev: fp16 [T, 3 * hidden], a token's row is Q | K | V, head h owns columns 64 h .. 64 h + 63 of each part. cu_dev: int32
 * [B + 1]; sequence b owns rows cu[b] .. cu[b + 1] - 1. dctx_dev: fp16 [T, hidden], the gradient of the context (under apex O1 the
 * out-projection's dgrad arrives in fp16, a loss scale riding in it). dqkv_dev: fp16 [T, 3 * hidden], laid out dQ | dK | dV like qkv;
 * every row of the call's sequences is written in full, nothing else is.
 *
 * Per (sequence, head), dO = the head's columns of dctx, s = Q K^T / 8, p = softmax(s) over the sequence's own keys:
 *     dV = p^T dO     dP = dO V^T     delta_i = sum_j p_ij dP_ij     dS = p o (dP - delta)     dQ = dS K / 8     dK = dS^T Q / 8
 * No dropout, no bias, no causal mask: the forward the product has.
 *
 * mode 0: every query. mode 3 (the retriever's last layer, whose forward computes only each sequence's first query): dctx_dev is fp16
 * [B, hidden]; dQ is written at row cu[b] and zeros in every other Q row; dK and dV of every key come from that single query.
 *
 * Rounding points. Operands are fp16 and their products exact in fp32; s and dP are fp32 sums of 64 products (v_mfma_f32_16x16x32_f16;
 * mode 3: fma chains); the log-sum-exp of a row, delta, p = exp(s - lse) and dS are fp32; p is rounded to fp16 only as the MFMA operand of
 * dV, dS only as the operand of dQ and dK; dQ, dK and dV accumulate in fp32, the factor 1/8 is applied to the fp32 sum, and every output
 * is rounded to fp16 once.
 *
 * No atomics: every output element has one owner and one summation order; two runs give the same bits, and a sequence's rows do not
 * depend on where in the batch it stands. No score, probability or dS matrix goes to memory; the workspace holds one (lse, delta) fp32
 * pair per (token, head) in mode 0 and nothing in mode 3. Non-finite inputs propagate by IEEE rules alone, inside their own sequence and
 * head; nothing faults.
 *
 * Limits: hidden == 64 * heads, 1 <= L <= 512, 1 <= B <= 65535. The lengths live on the device: the caller guarantees
 * cu[b + 1] - cu[b] <= L. A sequence of length 0 is skipped. What the host can see is validated: MDR_E_INVALID (a NULL or misaligned
 * pointer, a shape or mode outside the limits) or MDR_E_WORKSPACE (a short workspace), each with mdr_last_error() and without a launch.
 */
#ifndef MDR_ATTENTION_GRAD_H
#define MDR_ATTENTION_GRAD_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device scratch the call below needs: at most 16 * B * L * heads + 4096. 0 for an unsupported shape or mode, and for mode 3,
 * which needs none (workspace_dev may then be NULL). */
size_t mdr_attention_backward_workspace_bytes(int B, int L, int heads, int mode);

/* mode: 0 = every query, 3 = first query of each sequence. All pointers 16-byte aligned. */
int mdr_attention_backward(const void* qkv_dev, const void* dctx_dev, const int* cu_dev, int B, int L, int hidden, int heads, int mode, void* dqkv_dev,
                           void* workspace_dev, size_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_ATTENTION_GRAD_H */
