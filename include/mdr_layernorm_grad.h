/*
 * include/mdr_layernorm_grad.h -- C ABI of the backward of a LayerNorm of the trunk on packed rows in libmdrhip.so (gfx950), and of the
 * backward of the CLS gather. The forward is layernorm_kernel (csrc/mdr_encoder_pack_ln.inl, reachable as mdr_test_layernorm):
 *     y = (x - mu) * rstd * g + b,   x = in (+ res16 | res32),   mu = mean(x),   rstd = rsqrtf(mean((x - mu)^2) + eps)
 * The conventions of include/mdr_hip.h hold (int return codes, mdr_last_error(), *_dev = device pointers, `stream` = hipStream_t as void*,
 * caller-owned buffers, everything enqueued on `stream`, no synchronisation).
 *
 * Inputs. in_dev [M, H] fp32, or fp16 with in_f16 = 1; res16_dev fp16 [M, H] or res32_dev fp32 [M, H], at most one: exactly the forward's.
 * The forward saves nothing: x, mu and rstd are recomputed with the forward's expressions in the forward's order. The output gradient is
 *     dy = fp32(dy16) + fp32(dy2)        dy16_dev fp16 [M, H], dy2_dev fp16 [M, H] or fp32 with dy2_f32 = 1; either may be NULL, not both
 * (a LayerNorm output of the trunk feeds a Linear, whose dX comes back in fp16, and the next residual add, whose gradient comes back in fp16
 * or, with an fp32 residual stream, in fp32). g_dev fp32 [H]. m_dev is NULL or points to a device int, the number of valid rows (clamped to
 * 0 .. M), as in the forward. Rows at or behind it are never read as values and never written, and add nothing to dg or db.
 *
 * Per row, in fp32:   xhat = (x - mu) * rstd,   a = dy * g,   c1 = mean(a),   c2 = mean(a * xhat),   dx = rstd * (a - c1 - xhat * c2)
 * Outputs, each skipped when its pointer is NULL (at least one is required):
 *     dx16_dev fp16 [M, H], dx32_dev fp32 [M, H]   the same fp32 value, rounded once for dx16 and not at all for dx32; it is the gradient
 *                                                 of `in` and of the residual alike
 *     dg_dev fp32 [H]   the sum over the valid rows of dy * xhat
 *     db_dev fp32 [H]   the sum over the valid rows of dy
 * With accumulate != 0, dg and db are added to what the buffers hold: the old value enters last, in one fp32 add per element.
 * Outputs must not overlap inputs.
 *
 * No atomics: the rows are cut into S chunks of rows_per_chunk rows, a function of (M, H) alone. One workgroup of four waves owns a chunk;
 * wave w adds rows w, w + 4, ... of the chunk in order, the four waves are added in wave order, the chunks in a fixed order (sixteen
 * strands: strand j adds chunks j, j + 16, ... in order, then the strands are added in order), then the old value. Two runs give the same
 * bits, and a row's dx bits depend on that row's inputs and g only.
 * (csrc/mdr_layernorm_grad.hip lists the rounding points.)
 *
 * Limits: M >= 1, H a multiple of 64 with 64 <= H <= 1024, pointers 16-byte aligned. What the host can see is validated: MDR_E_INVALID (a
 * NULL in or g, both dy NULL, both residuals given, every output NULL, a flag that is neither 0 nor 1, a shape outside the limits, a
 * misaligned pointer) or MDR_E_WORKSPACE (a short workspace), each with mdr_last_error() and without a launch.
 */
#ifndef MDR_LAYERNORM_GRAD_H
#define MDR_LAYERNORM_GRAD_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_LAYERNORM_WANT_DG 1
#define MDR_LAYERNORM_WANT_DB 2

/* The split of the rows: a function of (M, H) ONLY (not of the device, not of *m_dev). Returns the number of chunks S >= 1 and stores the
 * rows of a chunk (a multiple of 4, S * rows_per_chunk >= M) in *rows_per_chunk (may be NULL). 0 (and *rows_per_chunk = 0) for a shape
 * outside the limits. */
int mdr_layernorm_backward_chunks(int M, int H, int* rows_per_chunk);

/* Bytes of device scratch mdr_layernorm_backward needs: the fp32 partial sums [S][2][H] when S > 1 and dg or db is wanted, else 0.
 * want: bit 0 dg, bit 1 db. 0 for a shape outside the limits. */
size_t mdr_layernorm_backward_workspace_bytes(int M, int H, int want);

int mdr_layernorm_backward(const void* in_dev, int in_f16, const void* res16_dev, const float* res32_dev, const void* dy16_dev,
                           const void* dy2_dev, int dy2_f32, int M, const int* m_dev, int H, const float* g_dev, float eps, void* dx16_dev,
                           float* dx32_dev, float* dg_dev, float* db_dev, int accumulate, void* workspace_dev, size_t workspace_bytes,
                           int device, void* stream);

/* The backward of the CLS gather (gather_cls_kernel): for every sequence b < B with cu[b + 1] > cu[b], row cu[b] of acc16_dev (fp16
 * [T, H], T = cu[B]) becomes fp16(fp32(acc) + fp32(d16[b])); d16_dev is fp16 [B, H], cu_dev int [B + 1]. No other row is touched and
 * empty sequences are skipped (the rule of mdr_attention_backward). Every row has one owner: no atomics. B >= 1, H as above. */
int mdr_gather_cls_backward(const void* d16_dev, const int* cu_dev, int B, int H, void* acc16_dev, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_LAYERNORM_GRAD_H */
