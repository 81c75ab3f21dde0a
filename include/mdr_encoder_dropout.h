/*
 * include/mdr_encoder_dropout.h -- C ABI of the inference encoder's training-mode forward in libmdrhip.so (gfx950): mdr_encoder_forward of
 * include/mdr_hip.h with the four dropout places of a training step live, for an encoder that is evaluated in train() mode but never
 * differentiated (the frozen key encoder of momentum training). Nothing is kept for a backward. The conventions of include/mdr_hip.h hold
 * (int return codes, mdr_last_error(), *_dev = device pointers, `stream` = hipStream_t as void*, caller-owned buffers, everything enqueued
 * on `stream`, no synchronisation, no atomics). The mask function, its thresholds and its rate are those of include/mdr_dropout.h.
 *
 * Places, per layer (layer 0 .. layers - 1) of encode `encode` (0 .. 5: which of a step's six encodes this is):
 *     place 0  emb   after the embedding LayerNorm (layer 0 only): h32 = LN(...) * m, h16 = fp16(h32)       hidden threshold
 *     place 1  attn  the attention probabilities (include/mdr_dropout.h: mode 0, the last layer mode 3)     attention threshold
 *     place 2  ao    after the out-projection, before the residual add: fp16(fp32(x16) * m)                 hidden threshold
 *     place 3  ff2   after FFN2, before the residual add: fp16(fp32(x16) * m)                               hidden threshold
 *     site = 1 + (encode * 64 + layer) * 4 + place
 * The hidden mask's row is the packed row (tokens whose mask is 0 dropped; in the last layer, whose tail runs on the first tokens alone,
 * the sequence's index), the attention mask's sequence is its index in the call: a sequence's output depends on its place in the batch,
 * so a batch is one call and cannot be sliced. ao and ff2 are folded into the LayerNorm that reads those rows, emb into the embedding
 * kernel: no separate pass over the hidden states is made. The bits are those of the training chain (dropout rows, then LayerNorm; the
 * embedding, then dropout rows) under the same (seed, site).
 *
 * A threshold of 0 makes its kind's places plain; with both 0 the call is mdr_encoder_forward, bit for bit. Only residual_fp32 = 2 (the
 * mode training is built for) is served: the other modes are refused with MDR_E_INVALID.
 */
#ifndef MDR_ENCODER_DROPOUT_H
#define MDR_ENCODER_DROPOUT_H

#include <stdint.h>

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mdr_encoder_forward with dropout. T_hidden, T_attention: 0 .. 255 (mdr_dropout_threshold of the two rates). encode: 0 .. 5. The handle has
 * at most 64 layers and residual_fp32 = 2; batch <= 65535. workspace: mdr_encoder_workspace_bytes(h, batch, seq_len), nothing more. */
int mdr_encoder_forward_dropout(mdr_encoder* h, const int64_t* ids_dev, const int64_t* mask_dev, int batch, int seq_len, int T_hidden, int T_attention,
                                uint64_t seed, int encode, float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Test hook: mdr_test_layernorm (fp16 in, optional res32) over fp32(fp16(fp32(in) * m)), m the hidden mask of (T, seed, site) at
 * (row, column). 0 <= T <= 255. Rows at or behind *rows_dev are not written. */
int mdr_test_layernorm_dropout(const void* in16_dev, const float* res32_dev, int rows_cap, const int* rows_dev, int H, const float* g_dev,
                               const float* b_dev, float eps, int T, uint64_t seed, uint32_t site, void* out16_dev, float* out32_dev, int device,
                               void* stream);

/* Test hook: mdr_test_embed_ln, flavour 0 (RoBERTa), with out32 = LN(...) * m and out16 = fp16(out32), m as above at (packed token, column). */
int mdr_test_embed_ln_dropout(const int64_t* ids_dev, const int* tok_src_dev, const int* tok_pid_dev, const int* total_dev, int cap,
                              const float* word_dev, const float* pos_dev, const float* type_dev, const float* g_dev, const float* b_dev, int H,
                              int vocab, int max_pos, float eps, int T, uint64_t seed, uint32_t site, void* out16_dev, float* out32_dev, int device,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_ENCODER_DROPOUT_H */
