/*
 * include/mdr_embedding_grad.h -- C ABI of the backward of the retriever's embedding layer on packed rows in libmdrhip.so (gfx950): the
 * gradients of the word table, the position table, the type row and the embedding LayerNorm's g and b. The forward is embed_ln_kernel
 * (csrc/mdr_encoder_pack_ln.inl, reachable as flavour 0 of mdr_test_embed_ln), for every packed token t < *total_dev:
 *     x = (word[clamp(ids[tok_src[t]], 0, vocab - 1)] + pos[min(tok_pid[t], max_pos - 1)]) + type0        y = (x - mu) * rstd * g + b
 * The conventions of include/mdr_hip.h hold (int return codes, mdr_last_error(), *_dev = device pointers, `stream` = hipStream_t as void*,
 * caller-owned buffers, everything enqueued on `stream`, no synchronisation). The token count is the device int *total_dev (clamped to
 * 0 .. cap) and is never read on the host: every grid is sized by `cap` (a forward passes B * L) and exits early.
 *
 * The table gradients are a scatter-add over token ids. Its order depends on the ids alone, so the sort is a PLAN, built once per forward
 * (mdr_embedding_plan), and the backward is a segmented sum in ascending token order (mdr_embedding_scatter, or fused behind the LayerNorm
 * backward: mdr_embedding_backward). No floating-point atomics anywhere; two runs give the same bits.
 *
 * The plan buffer: int32 words, C = cap, TS = (3 C + 1 rounded up to a multiple of 4)
 *     [0]  MDR_EMBEDDING_PLAN_MAGIC   [1] total (clamped to 0 .. C)   [2] number of word segments   [3] number of position segments
 *     [4]  C   [5] vocab   [6] max_pos   [7] pad_row   [8 .. 15] 0
 *     word table at W = 16, position table at W = 16 + TS, each:
 *         W           order[C]         the tokens t < total in STABLE order of their clamped row: ascending row, ascending t within a row
 *         W + C       seg_start[C + 1] segment s is order[seg_start[s] .. seg_start[s + 1]); seg_start[number of segments] = total
 *         W + 2 C + 1 seg_row[C]       the table row of segment s, ascending in s; a segment whose row is pad_row is SKIPPED and holds
 *                                      -1 - row instead (Hugging Face's padding_idx: that row of each table receives no gradient;
 *                                      pad_row = -1 disables the rule)
 *     16 + 2 TS       key_word[C], key_pos[C]   the clamped row of token t (scratch of the sort; valid for t < total)
 * Entries behind `total` (order), behind the number of segments (seg_row) and behind the number of segments + 1 (seg_start) are not
 * written. Rows are clamped as the forward reads them: ids below 0 join row 0, ids >= vocab row vocab - 1, tok_pid >= max_pos row
 * max_pos - 1 (and a negative tok_pid, which the forward does not allow, row 0). The plan is a pure function of the integer inputs.
 * The sort ranks by counting: the rank of t is the number of t' whose (row, t') is smaller; its work grows with total^2 (it is meant for
 * the batch of one forward, and to be enqueued at forward time, off the backward's critical path).
 *
 * The segmented sum. One workgroup owns a segment, hence one owner per output element. A segment's d rows are added in ascending t, in
 * PIECES of MDR_EMBEDDING_PIECE tokens: piece k of a segment of n tokens is its tokens k P .. min((k + 1) P, n) - 1 (a function of n
 * alone), a piece is summed from 0 in token order, the pieces are added from 0 in ascending piece order, the old value enters last
 * (accumulate). A table row's bits therefore depend on the d rows of its own tokens in token order only, not on the other tokens.
 *     accumulate = 0: EVERY row of each given table is written: +0 where no token has the row and for pad_row.
 *     accumulate = 1: only rows that own a segment that is not skipped are touched: new = sum + old, one fp32 add per element.
 * dtype0 (and dg, db of mdr_embedding_backward) are sums over all valid tokens under the split of include/mdr_layernorm_grad.h: the cap
 * rows are cut into S chunks of rows_per_chunk rows (mdr_embedding_backward_chunks, a function of (cap, H) alone), wave w of a chunk's
 * workgroup adds rows w, w + 4, ... in order, the four waves are added in wave order, the chunks in sixteen strands (strand j adds chunks
 * j, j + 16, ... in order, then the strands in order), then the old value. pad_row does not apply to them.
 *
 * Limits: 1 <= cap <= 2^20, 1 <= vocab <= 2^20, 1 <= max_pos <= 2^16, -1 <= pad_row < 2^20, H a multiple of 64 with 64 <= H <= 1024,
 * float, plan and workspace pointers 16-byte aligned. What the host can see is validated: MDR_E_INVALID or MDR_E_WORKSPACE (a short plan
 * or workspace buffer), each with mdr_last_error() and without a launch. mdr_embedding_scatter and mdr_embedding_backward must be given
 * the cap, vocab and max_pos the plan was built with; a plan whose header disagrees makes the table kernels do nothing.
 * Outputs must not overlap inputs.
 */
#ifndef MDR_EMBEDDING_GRAD_H
#define MDR_EMBEDDING_GRAD_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_EMBEDDING_PIECE 16              /* P: tokens of a piece of a segment */
#define MDR_EMBEDDING_PLAN_HEADER 16        /* int32 words in front of the word table's section */
#define MDR_EMBEDDING_PLAN_MAGIC 0x4D455031 /* "MEP1" */

/* Bytes of a plan buffer for `cap` tokens: a function of cap only. 0 for a cap outside the limits. */
size_t mdr_embedding_plan_bytes(int cap);

/* Builds the plan for ids_dev (i64, indexed by tok_src), tok_src_dev and tok_pid_dev (i32 [cap]; entries from *total_dev on are never
 * read). Three launches. */
int mdr_embedding_plan(const int64_t* ids_dev, const int* tok_src_dev, const int* tok_pid_dev, const int* total_dev, int cap, int vocab,
                       int max_pos, int pad_row, void* plan_dev, size_t plan_bytes, int device, void* stream);

/* The split of the cap rows for dtype0, dg and db: the number of chunks S >= 1, and the rows of a chunk (a multiple of 4, S *
 * rows_per_chunk >= cap) in *rows_per_chunk (may be NULL). A function of (cap, H) ONLY. 0 (and 0) for a shape outside the limits. */
int mdr_embedding_backward_chunks(int cap, int H, int* rows_per_chunk);

/* Bytes of device scratch of mdr_embedding_scatter: the partial sums [S][H] of dtype0. 0 for a shape outside the limits. */
size_t mdr_embedding_scatter_workspace_bytes(int cap, int H);

/* d32_dev fp32 [cap, H], the gradient of x; rows at or behind the plan's total are never read as values. dword_dev fp32 [vocab, H],
 * dpos_dev fp32 [max_pos, H], dtype0_dev fp32 [H]: each may be NULL, not all three. */
int mdr_embedding_scatter(const float* d32_dev, const void* plan_dev, int cap, int H, int vocab, int max_pos, float* dword_dev,
                          float* dpos_dev, float* dtype0_dev, int accumulate, void* workspace_dev, size_t workspace_bytes, int device,
                          void* stream);

/* Bytes of device scratch of mdr_embedding_backward: d in fp32 [cap, H] and the partial sums [S][3][H]. 0 outside the limits. */
size_t mdr_embedding_backward_workspace_bytes(int cap, int H);

/* The LayerNorm backward fused with the gather, then the scatter. Per token t < total the kernel recomputes x, mu and rstd from the
 * tables with the forward's expressions in the forward's order, forms dy = fp32(dy16) + fp32(dy2) (dy16_dev fp16 [cap, H], dy2_dev fp16
 * or, with dy2_f32 = 1, fp32 [cap, H]; either may be NULL, not both),
 *     xhat = (x - mu) * rstd,   a = dy * g,   c1 = mean(a),   c2 = mean(a * xhat),   d = rstd * ((a - c1) - xhat * c2)
 * as mdr_layernorm_backward does, and writes d in fp32 to the workspace -- or, when d32_dev fp32 [cap, H] is given, there instead, so that
 * the two halves can be checked apart (rows at or behind total are not written). Outputs, each skipped when NULL (at least one of them or
 * d32_dev):
 *     dword_dev, dpos_dev: the segmented sums of d;   dtype0_dev fp32 [H]: the sum of d over the valid tokens
 *     dg_dev fp32 [H]: the sum of dy * xhat;   db_dev fp32 [H]: the sum of dy
 * all under `accumulate` as above. (csrc/mdr_embedding_grad.hip lists the rounding points.) */
int mdr_embedding_backward(const int64_t* ids_dev, const int* tok_src_dev, const int* tok_pid_dev, const int* total_dev, int cap,
                           const float* word_dev, const float* pos_dev, const float* type0_dev, const float* g_dev, int H, int vocab,
                           int max_pos, float eps, const void* dy16_dev, const void* dy2_dev, int dy2_f32, const void* plan_dev,
                           float* dword_dev, float* dpos_dev, float* dtype0_dev, float* dg_dev, float* db_dev, float* d32_dev,
                           int accumulate, void* workspace_dev, size_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_EMBEDDING_GRAD_H */
