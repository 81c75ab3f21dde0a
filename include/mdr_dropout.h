/*
 * include/mdr_dropout.h -- C ABI of dropout for the training bricks in libmdrhip.so (gfx950): a replayable Philox4x32-10 mask for hidden
 * states (packed rows) and for attention probabilities (a training attention forward and the backward that replays its mask). The
 * conventions of include/mdr_hip.h hold (int return codes, mdr_last_error(), *_dev = device pointers, `stream` = hipStream_t as void*,
 * caller-owned buffers, everything enqueued on `stream`, no synchronisation, no atomics).
 *
 * The mask is a pure function of (seed, site, the element's indices, T) and of nothing else: not of L, the launch geometry, which pass
 * asks, or the rest of the batch. Nothing is stored: the backward draws the forward's mask again.
 *   generator  Philox4x32-10 (Salmon et al., SC 2011): multipliers 0xD2511F53 and 0xCD9E8D57, Weyl constants 0x9E3779B9 and 0xBB67AE85,
 *              key (seed & 0xffffffff, seed >> 32). One call yields four words = 16 bytes; byte k = (word[k >> 2] >> (8 (k & 3))) & 0xff.
 *   threshold  T = floor(256 p + 0.5); an element is kept iff its byte >= T. T = 0 is no dropout. A p outside [0, 1) or one with T = 256 is
 *              invalid.
 *   rate       The rate drawn is p_eff = T / 256, not the nominal p: p = 0.1 draws 26 / 256 = 0.1016 (eight bits per element: one
 *              generator call per 16 hidden elements or per 4 x 4 block of probabilities). The scale of a kept element is
 *              fp32(256 / (256 - T)): the expectation is exact for the rate actually drawn.
 *   factor     The mask value m is 0 or the scale and is applied as an IEEE multiplication, never as a select: a non-finite value at a
 *              dropped position becomes NaN, as torch's x * mask makes it, so an overflow is never hidden by a drop.
 *   hidden     Element (row, col) of an [M, N] tensor, N a multiple of 16: byte col & 15 of counter (col >> 4, row, 0, site).
 *   attention  The probability of query i, key j (both sequence-local), head h, sequence b (the index in the call's cu): byte
 *              4 (i & 3) + (j & 3) of counter (i >> 2, j >> 2, b * heads + h, site). Mode 3 is the same function at i = 0. The mask
 *              depends on b: with dropout a sequence's context and gradient depend on its place in the batch, as torch's do.
 *   uniqueness It is the CALLER's duty to give every use its own site or seed: every step, encode, layer and place. Two uses that share
 *              (seed, site) share their mask.
 *
 * Attention: layout, modes and limits are those of include/mdr_attention_grad.h (qkv fp16 [T, 3 * hidden], cu int32 [B + 1], head dim 64,
 * 1 <= L <= 512, 1 <= B <= 65535, mode 0 = every query, mode 3 = the first query of each sequence; the caller guarantees
 * cu[b + 1] - cu[b] <= L; a sequence of length 0 is skipped). With p = softmax(Q K^T / 8) and Pd = p o m:
 *     ctx = Pd V      dV = Pd^T dO      dP = (dO V^T) o m      delta_i = sum_j p_ij dP_ij      dS = p o (dP - delta)
 *     dQ = dS K / 8   dK = dS^T Q / 8
 * Rounding points: those of include/mdr_attention_grad.h, and: dP o m and p o m are fp32 products; Pd is rounded to fp16 only as the operand of
 * ctx and dV; ctx accumulates in fp32 and is rounded to fp16 once. No probability goes to memory.
 *
 * What the host can see is validated before any launch: MDR_E_INVALID (a NULL or misaligned pointer, a shape, mode or T outside the
 * limits) or MDR_E_WORKSPACE (a short workspace), each with mdr_last_error().
 */
#ifndef MDR_DROPOUT_H
#define MDR_DROPOUT_H

#include <stdint.h>

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* T = floor(256 p + 0.5) in 0 .. 255, or -1 for an invalid p (outside [0, 1), NaN, or T = 256). */
int mdr_dropout_threshold(float p);

/* Test hook: out_dev (uint8 [n0, n1, 16]) receives the 16 bytes of counter (c0, c1, c2, site) under the key of `seed` for every c0 < n0,
 * c1 < n1. 1 <= n0, n1 <= 65536. */
int mdr_test_dropout_bytes(uint64_t seed, uint32_t c2, uint32_t site, int n0, int n1, void* out_dev, int device, void* stream);

/* y = (x + add16) * m on packed rows [M, N], N a multiple of 16, the hidden site. x_dev: fp16 (x_is_fp16) or fp32. add16_dev: NULL, or for an
 * fp32 x an fp16 [M, N] tensor added in fp32 before the mask (the backward of a forward that returned y16 as well: two gradients, one mask).
 * rows_dev: NULL or an int32 device scalar, the number of valid rows: rows at or behind it are neither read as values nor written. y_dev has
 * x's dtype; y16_dev: NULL, or for an fp32 x a second output fp16(y) (one mask, one rounding of the fp32 y). 0 <= T <= 255 (T = 0: m = 1).
 * The backward of y = x * m is the same call on the gradient with the same (T, seed, site). All pointers 16-byte aligned. */
int mdr_dropout_rows(const void* x_dev, int x_is_fp16, const void* add16_dev, int M, const int* rows_dev, int N, int T, uint64_t seed, uint32_t site,
                     void* y_dev, void* y16_dev, int device, void* stream);

/* ctx = (softmax(Q K^T / 8) o m) V. ctx_dev: fp16 [T, hidden] (mode 0) or [B, hidden] (mode 3); rows of the call's non-empty sequences are
 * written, nothing else. 1 <= T <= 255: T = 0 is refused (the caller uses the forward without dropout, whose bits the encoder owns). */
int mdr_attention_dropout_forward(const void* qkv_dev, const int* cu_dev, int B, int L, int hidden, int heads, int mode, int T, uint64_t seed,
                                  uint32_t site, void* ctx_dev, int device, void* stream);

/* The backward of the call above with the same (T, seed, site): dqkv_dev as mdr_attention_backward writes it, workspace as
 * mdr_attention_backward_workspace_bytes(B, L, heads, mode) of include/mdr_attention_grad.h says. */
int mdr_attention_dropout_backward(const void* qkv_dev, const void* dctx_dev, const int* cu_dev, int B, int L, int hidden, int heads, int mode, int T,
                                   uint64_t seed, uint32_t site, void* dqkv_dev, void* workspace_dev, size_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_DROPOUT_H */
