/*
 * include/mdr_head_grad.h -- C ABI of the backward of the retriever's head Linear (project.0) in libmdrhip.so (gfx950): the gradients of
 *     Y[M, N] = X[M, K] W[N, K]^T + b[N],   Y kept in fp32 (the forward is mdr_test_gemm_f16 with epilogue 3, the encoder's EPI_BIAS_F32)
 * with respect to X, W and b, from an fp32 dY. The conventions of include/mdr_hip.h hold (int return codes, mdr_last_error(), *_dev = device
 * pointers, `stream` = hipStream_t as void*, caller-owned buffers, everything enqueued on `stream`, no synchronisation).
 *
 * Layout. x_dev fp16 [M, K], w_dev fp16 [N, K], dy_dev fp32 [M, N], row-major and contiguous. Every one of the M rows is valid: the head
 * runs on the B CLS rows of a batch, so there is no device row count.
 *
 * Outputs, each skipped when its pointer is NULL:
 *     dx_dev fp16 [M, K]   dX = fp16(dY W)
 *     dw_dev fp32 [N, K]   dW = dY^T X
 *     db_dev fp32 [N]      db = the column sums of dY
 * With accumulate != 0, dW and db are added to what the buffers hold: the old value enters last, in one fp32 add per element.
 *
 * Rounding points. dY is fp32 and is never rounded to fp16. Every product and sum is an fp32 fused multiply-add; dX is rounded to fp16
 * once; dW and db are not rounded again. A non-finite dY element reaches row m of dX, row n of dW and element n of db as a non-finite
 * value: it is multiplied by the operand as it stands, never by a mask. (csrc/mdr_head_grad.hip has the full list and the orders.)
 *
 * No atomics: the rows are split into S = ceil(M / 128) chunks, a function of M alone; every output element has one owner and one
 * summation order (the rows of a chunk in order, the chunks in order, then the old value), so two runs give the same bits.
 *
 * Limits: M >= 1, N and K positive multiples of 64, pointers 16-byte aligned. What the host can see is validated: MDR_E_INVALID (a NULL x,
 * w or dy, all three outputs NULL, a shape outside the limits, a misaligned pointer) or MDR_E_WORKSPACE (a short workspace), each with
 * mdr_last_error() and without a launch.
 */
#ifndef MDR_HEAD_GRAD_H
#define MDR_HEAD_GRAD_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_HEAD_WANT_DX 1
#define MDR_HEAD_WANT_DW 2
#define MDR_HEAD_WANT_DB 4

/* Bytes of device scratch mdr_head_backward needs: the chunks' partial sums of dW and db when M > 128, nothing otherwise.
 * want: bit 0 dX, bit 1 dW, bit 2 db. 0 for a shape outside the limits. */
size_t mdr_head_backward_workspace_bytes(int M, int N, int K, int want);

int mdr_head_backward(const void* x_dev, const void* w_dev, const float* dy_dev, int M, int N, int K, void* dx_dev, float* dw_dev,
                      float* db_dev, int accumulate, void* workspace_dev, size_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_HEAD_GRAD_H */
