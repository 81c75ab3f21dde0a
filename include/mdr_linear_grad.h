/*
 * include/mdr_linear_grad.h -- C ABI of the backward of a Linear of the trunk on packed rows in libmdrhip.so (gfx950): the gradients of
 *     Y[M, N] = act(X[M, K] W[N, K]^T + b[N]),   act = identity or erf-GELU
 * with respect to X, W and b. The conventions of include/mdr_hip.h hold (int return codes, mdr_last_error(), *_dev = device pointers,
 * `stream` = hipStream_t as void*, caller-owned buffers, everything enqueued on `stream`, no synchronisation).
 *
 * Layout. x_dev fp16 [M, K], w_dev fp16 [N, K], dy_dev fp16 [M, N], row-major and contiguous: the layout of mdr_test_gemm_f16. m_dev is
 * NULL or points to a device int, the number of valid rows (clamped to 0 .. M), as in the forward. Rows at or behind it are never read as
 * values: they are zero-filled on load, not multiplied by zero, so a NaN there changes nothing. pre_dev is NULL for the identity;
 * otherwise it is the fp16 pre-activation u = fp16(X W^T + b) [M, N], and the call first forms dZ = fp16(dY * gelu'(u)) in the workspace
 * (valid rows; the others zero) and uses dZ wherever dY stands below. gelu'(u) = Phi(u) + u phi(u) in fp32.
 *
 * Outputs, each skipped when its pointer is NULL:
 *     dx_dev fp16 [M, K]   dX = dY W        rows at or behind the valid count are not written
 *     dw_dev fp32 [N, K]   dW = dY^T X
 *     db_dev fp32 [N]      db = the column sums of dY
 * With accumulate != 0, dW and db are added to what the buffers hold: the old value enters last, in one fp32 add per element.
 *
 * Rounding points. Operands are fp16 and their products exact in fp32; every sum accumulates in fp32; dX and dZ are rounded to fp16 once;
 * dW and db are not rounded again. (csrc/mdr_linear_grad.inl has the full list.)
 *
 * No atomics: the token rows are split into S chunks of rows_per_chunk rows, a function of (M, N, K) alone; every output element has one
 * owner and one summation order (slabs in row order inside a chunk, chunks in order, then the old value), so two runs give the same bits.
 *
 * Limits: M >= 1, N and K positive multiples of 64 (the forward hook's rule), pointers 16-byte aligned. What the
 * host can see is validated: MDR_E_INVALID (a NULL x, w or dy, all three outputs NULL, a shape outside the limits, a misaligned pointer)
 * or MDR_E_WORKSPACE (a short workspace), each with mdr_last_error() and without a launch.
 */
#ifndef MDR_LINEAR_GRAD_H
#define MDR_LINEAR_GRAD_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_LINEAR_WANT_DX 1
#define MDR_LINEAR_WANT_DW 2
#define MDR_LINEAR_WANT_DB 4
#define MDR_LINEAR_WANT_PRE 8

/* The split of the token rows the weight-gradient and bias-gradient kernels use: a function of (M, N, K) ONLY (not of the device, not of
 * *m_dev). Returns the number of chunks S >= 1 and stores the rows of a chunk (a multiple of 64) in *rows_per_chunk (may be NULL).
 * 0 (and *rows_per_chunk = 0) for a shape outside the limits. */
int mdr_linear_backward_chunks(int M, int N, int K, int* rows_per_chunk);

/* Bytes of device scratch mdr_linear_backward needs. want: bit 0 dX, bit 1 dW, bit 2 db, bit 3 a pre-activation is given.
 * 0 for a shape outside the limits. */
size_t mdr_linear_backward_workspace_bytes(int M, int N, int K, int want);

int mdr_linear_backward(const void* x_dev, const void* w_dev, const void* dy_dev, const void* pre_dev, int M, const int* m_dev, int N, int K,
                        void* dx_dev, float* dw_dev, float* db_dev, int accumulate, void* workspace_dev, size_t workspace_bytes, int device,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_LINEAR_GRAD_H */
