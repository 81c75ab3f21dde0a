/*
 * include/mdr_reader_embedding_grad.h -- C ABI of the backward of the READER's embedding layer on packed rows in libmdrhip.so (gfx950): the
 * ELECTRA / BERT flavour of include/mdr_embedding_grad.h, whose conventions, limits, plan layout, segmented sum and chunk split hold here
 * unless said otherwise. The forward is reader_embed_ln_kernel (csrc/mdr_reader.inl, reachable as flavour 1 of mdr_test_embed_ln), for
 * every packed token t < *total_dev:
 *     x = (word[clamp(ids[tok_src[t]], 0, vocab - 1)] + pos[tok_src[t] % L]) + type[ty]        y = (x - mu) * rstd * g + b
 *     ty = clamp(types[tok_src[t]], 0, type_vocab - 1), or 0 when types is NULL;  the caller guarantees L <= max_pos
 * It differs from the retriever's flavour in three places. The position is absolute within the row and comes from tok_src, not from
 * tok_pid. The type embedding is a [type_vocab, H] table, and its gradient dtype [type_vocab, H] has one row per type id. And the pad row
 * is given PER TABLE: Hugging Face's ElectraEmbeddings gives word_embeddings padding_idx = pad_token_id (0) and the position table none --
 * position row 0 is every sequence's [CLS] and must receive its gradient, so a reader passes pad_pos = -1.
 *
 * The plan has the layout of include/mdr_embedding_grad.h (mdr_embedding_plan_bytes sizes it) and its own kind:
 *     [0] MDR_READER_EMBEDDING_PLAN_MAGIC   [1] total   [2] word segments   [3] position segments   [4] cap   [5] vocab   [6] max_pos
 *     [7] pad_word   [8] pad_pos   [9] L   [10 .. 15] 0
 * The position keys are tok_src[t] % L: at most L distinct rows, row p owning one token of every sequence longer than p, in ascending t.
 * A segment of the word table whose row is pad_word, and one of the position table whose row is pad_pos, is skipped (-1 - row in seg_row).
 * A plan of one kind given to the other kind's scatter or backward makes the table kernels do nothing, as a header that disagrees in cap,
 * vocab, max_pos (or, here, L) does.
 *
 * dtype[k] is the sum of d over the valid tokens whose ty is k, under the chunk, wave and strand split of dtype0, dg and db
 * (mdr_embedding_backward_chunks: a function of (cap, H) alone); a token adds to its own row's sum only, so row k has the bits of the
 * retriever's dtype0 over the tokens of type k with the others' d replaced by nothing. 1 <= type_vocab <= MDR_READER_EMBEDDING_MAX_TYPES.
 * No floating-point atomics, one owner per output element: two runs give the same bits.
 */
#ifndef MDR_READER_EMBEDDING_GRAD_H
#define MDR_READER_EMBEDDING_GRAD_H

#include "mdr_embedding_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_READER_EMBEDDING_PLAN_MAGIC 0x4D455032 /* "MEP2" */
#define MDR_READER_EMBEDDING_MAX_TYPES 4           /* rows of the type table the backward keeps sums for */

/* Builds the reader's plan for ids_dev (i64, indexed by tok_src) and tok_src_dev (i32 [cap]; entries from *total_dev on are never read).
 * 1 <= L <= max_pos; pad_word in -1 .. 2^20 - 1, pad_pos in -1 .. 2^16 - 1 (-1: the table has no pad row). plan_bytes >=
 * mdr_embedding_plan_bytes(cap). Three launches. */
int mdr_reader_embedding_plan(const int64_t* ids_dev, const int* tok_src_dev, const int* total_dev, int cap, int L, int vocab, int max_pos,
                              int pad_word, int pad_pos, void* plan_dev, size_t plan_bytes, int device, void* stream);

/* Bytes of device scratch of mdr_reader_embedding_backward: d in fp32 [cap, H], the partial sums [S][2][H] of dg and db and [S][type_vocab][H]
 * of dtype. 0 outside the limits. */
size_t mdr_reader_embedding_backward_workspace_bytes(int cap, int H, int type_vocab);

/* mdr_embedding_backward for the forward above: types_dev i64 (indexed by tok_src) or NULL, type_dev fp32 [type_vocab, H]. Outputs, each
 * skipped when NULL (at least one of them or d32_dev), each under `accumulate` with the semantics of include/mdr_embedding_grad.h:
 *     dword_dev fp32 [vocab, H], dpos_dev fp32 [max_pos, H]: the segmented sums of d (they need the reader's plan, built with this L)
 *     dtype_dev fp32 [type_vocab, H]: row k the sum of d over the valid tokens of type k (+0 where no token has the type)
 *     dg_dev fp32 [H]: the sum of dy * xhat;   db_dev fp32 [H]: the sum of dy;   d32_dev fp32 [cap, H]: d, rows behind total not written
 * (csrc/mdr_embedding_grad.hip lists the rounding points.) */
int mdr_reader_embedding_backward(const int64_t* ids_dev, const int64_t* types_dev, const int* tok_src_dev, const int* total_dev, int cap, int L,
                                  const float* word_dev, const float* pos_dev, const float* type_dev, int type_vocab, const float* g_dev, int H,
                                  int vocab, int max_pos, float eps, const void* dy16_dev, const void* dy2_dev, int dy2_f32, const void* plan_dev,
                                  float* dword_dev, float* dpos_dev, float* dtype_dev, float* dg_dev, float* db_dev, float* d32_dev, int accumulate,
                                  void* workspace_dev, size_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_READER_EMBEDDING_GRAD_H */
