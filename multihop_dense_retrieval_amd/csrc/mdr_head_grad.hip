// csrc/mdr_head_grad.hip -- the backward of the retriever's head Linear (include/mdr_head_grad.h: mdr_head_backward):
//     Y[M, N] = X[M, K] W[N, K]^T + b[N] with Y in fp32:   dX = fp16(dY W)   dW = dY^T X   db = column sums of dY,   dY fp32.
// The forward is the encoder's own GEMM (EPI_BIAS_F32); only the backward lives here. At the training batch (M = 150, N = K = 768) the whole
// call is 0.35 GFLOP, so the kernels are plain fp32 FMA loops on the vector unit with no LDS and no MFMA: nothing here is tuned.
//
// hg_dx_kernel      a workgroup of 4 waves owns 16 rows x 64 columns of dX; a thread owns one column k and 4 rows and walks n = 0 .. N - 1
//                   in order: acc[r] = fma(dY[m_r, n], fp32(W[n, k]), acc[r]). The W row is read once per 4 rows, coalesced over k; dY[m, n] is
//                   the same address across a wave. Rows at or behind M are neither loaded nor stored.
// hg_dw_kernel      a workgroup owns 16 rows (n) x 64 columns (k) of dW and one chunk of 128 token rows; a thread owns one k and 4
//                   consecutive n and walks the chunk's rows in order: acc[j] = fma(dY[m, n_j], fp32(X[m, k]), acc[j]). With S > 1 chunks
//                   the tile goes to the fp32 workspace [S][N][K].
// hg_db_kernel      a thread owns one column n of one chunk: acc += dY[m, n] over the chunk's rows in order. With S > 1: workspace [S][N].
// hg_reduce_kernel  out = partial[0] + partial[1] + ... + partial[S - 1] (in this order), then + the old value if `accumulate`.
// Every output element has one owner and one summation order: no atomics, and two runs give the same bits.
//
// Rounding points (tests/head_grad_ref.py derives its bound from this list):
//   1. x and w are fp16, dy is fp32: exact operands, widened to fp32. dy is never rounded to fp16. A product dy * w or dy * x is NOT exact in
//      fp32 (24 x 11 bits); it is never formed on its own: each step is one v_fma_f32, one rounding of acc + product.
//   2. dX[m, k]: N fused steps in the order n = 0 .. N - 1 from acc = 0, then ONE rounding to fp16 (round to nearest even; beyond the fp16
//      range: infinity).
//   3. dW[n, k]: the rows of a chunk in order from acc = 0, the S chunks added in order in fp32, then the old value: no further rounding.
//   4. db[n]: fp32 adds in the same orders: no further rounding.
//   A non-finite dy[m, n] enters acc through an fma with the operand as it stands (inf * 0 is NaN, still non-finite) and nothing resets acc,
//   so it arrives in row m of dX, row n of dW and element n of db; no other row or element reads it.

#include "mdr_common.h"
#include "../../include/mdr_head_grad.h"

namespace mdr {
namespace {

constexpr int kHgCols = 64;      // output columns of a workgroup: one per lane
constexpr int kHgPer = 4;        // rows of the output tile a thread owns
constexpr int kHgWaves = 4;
constexpr int kHgThreads = kHgCols * kHgWaves;
constexpr int kHgTileRows = kHgPer * kHgWaves;  // 16
constexpr int kHgChunk = 128;    // token rows per chunk of the dW / db sums: S = ceil(M / 128), a function of M alone

// grid (K / 64, ceil(M / 16))
__global__ void __launch_bounds__(kHgThreads)
hg_dx_kernel(const float* __restrict__ dy, const _Float16* __restrict__ w, int M, int N, int K, _Float16* __restrict__ dx) {
    const int k = blockIdx.x * kHgCols + (threadIdx.x & (kHgCols - 1));
    const int m0 = blockIdx.y * kHgTileRows + (threadIdx.x >> 6) * kHgPer;
    if (m0 >= M) return;
    const int rows = min(kHgPer, M - m0);
    float acc[kHgPer] = {0.f, 0.f, 0.f, 0.f};
    const float* d = dy + (size_t)m0 * N;
    for (int n = 0; n < N; ++n) {
        const float wv = (float)w[(size_t)n * K + k];
#pragma unroll
        for (int r = 0; r < kHgPer; ++r)
            if (r < rows) acc[r] = __builtin_fmaf(d[(size_t)r * N + n], wv, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kHgPer; ++r)
        if (r < rows) dx[(size_t)(m0 + r) * K + k] = (_Float16)acc[r];
}

// grid (K / 64, N / 16, S). out: dw itself (S == 1) or the partials [S][N][K].
__global__ void __launch_bounds__(kHgThreads)
hg_dw_kernel(const float* __restrict__ dy, const _Float16* __restrict__ x, int M, int N, int K, float* __restrict__ out, int add_old) {
    const int k = blockIdx.x * kHgCols + (threadIdx.x & (kHgCols - 1));
    const int n0 = blockIdx.y * kHgTileRows + (threadIdx.x >> 6) * kHgPer;  // N is a multiple of 64: the four n are inside
    const int chunk = blockIdx.z;
    const int row_begin = chunk * kHgChunk, row_end = min(row_begin + kHgChunk, M);
    float acc[kHgPer] = {0.f, 0.f, 0.f, 0.f};
    for (int m = row_begin; m < row_end; ++m) {
        const float xv = (float)x[(size_t)m * K + k];
        const float* d = dy + (size_t)m * N + n0;
#pragma unroll
        for (int j = 0; j < kHgPer; ++j) acc[j] = __builtin_fmaf(d[j], xv, acc[j]);
    }
    float* o = out + (size_t)chunk * (size_t)N * (size_t)K;
#pragma unroll
    for (int j = 0; j < kHgPer; ++j) {
        float* p = o + (size_t)(n0 + j) * K + k;
        float v = acc[j];
        if (add_old) v += *p;
        *p = v;
    }
}

// grid (N / 64, S), 64 threads. out: db itself (S == 1) or the partials [S][N].
__global__ void __launch_bounds__(kHgCols)
hg_db_kernel(const float* __restrict__ dy, int M, int N, float* __restrict__ out, int add_old) {
    const int n = blockIdx.x * kHgCols + threadIdx.x;
    const int chunk = blockIdx.y;
    const int row_begin = chunk * kHgChunk, row_end = min(row_begin + kHgChunk, M);
    float acc = 0.f;
    for (int m = row_begin; m < row_end; ++m) acc += dy[(size_t)m * N + n];
    float* p = out + (size_t)chunk * N + n;
    if (add_old) acc += *p;
    *p = acc;
}

// out[i] = part[0][i] + part[1][i] + ... + part[S - 1][i] (+ out[i] last)
__global__ void __launch_bounds__(256)
hg_reduce_kernel(const float* __restrict__ part, int S, size_t count, float* __restrict__ out, int add_old) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    float t = part[i];
    for (int s = 1; s < S; ++s) t += part[(size_t)s * count + i];
    if (add_old) t += out[i];
    out[i] = t;
}

struct HgPlan {
    int S = 0;
    size_t off_dwp = 0, off_dbp = 0, bytes = 0;
};

bool hg_shape_ok(int M, int N, int K) { return M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0; }

HgPlan hg_plan(int M, int N, int K, int want) {
    HgPlan p;
    p.S = (M + kHgChunk - 1) / kHgChunk;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align_up(bytes, 256); return o; };
    if ((want & MDR_HEAD_WANT_DW) && p.S > 1) p.off_dwp = take((size_t)p.S * N * K * 4);
    if ((want & MDR_HEAD_WANT_DB) && p.S > 1) p.off_dbp = take((size_t)p.S * N * 4);
    p.bytes = at;
    return p;
}

}  // namespace
}  // namespace mdr

using namespace mdr;

extern "C" {

size_t mdr_head_backward_workspace_bytes(int M, int N, int K, int want) {
    if (!hg_shape_ok(M, N, K)) return 0;
    return hg_plan(M, N, K, want).bytes;
}

int mdr_head_backward(const void* x_dev, const void* w_dev, const float* dy_dev, int M, int N, int K, void* dx_dev, float* dw_dev,
                      float* db_dev, int accumulate, void* workspace_dev, size_t workspace_bytes, int device, void* stream) {
    MDR_REQUIRE(x_dev && w_dev && dy_dev, "NULL pointer: x, w and dy are required");
    MDR_REQUIRE(dx_dev || dw_dev || db_dev, "nothing to compute: dx, dw and db are all NULL");
    MDR_REQUIRE(M >= 1, "M=%d must be at least 1", M);
    MDR_REQUIRE(N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0, "bad Linear shape N=%d K=%d (positive multiples of 64)", N, K);
    MDR_REQUIRE(aligned16({x_dev, w_dev, dy_dev, dx_dev, dw_dev, db_dev, workspace_dev}), "pointers must be 16-byte aligned");
    const int want = (dx_dev ? MDR_HEAD_WANT_DX : 0) | (dw_dev ? MDR_HEAD_WANT_DW : 0) | (db_dev ? MDR_HEAD_WANT_DB : 0);
    const HgPlan p = hg_plan(M, N, K, want);
    MDR_REQUIRE_WORKSPACE("mdr_head_backward", workspace_dev, workspace_bytes, p.bytes, "mdr_head_backward_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace_dev;
    const _Float16* x = (const _Float16*)x_dev;
    const _Float16* w = (const _Float16*)w_dev;
    const int add_old = accumulate ? 1 : 0;

    if (dx_dev) {
        hipLaunchKernelGGL(hg_dx_kernel, dim3(K / kHgCols, (M + kHgTileRows - 1) / kHgTileRows), dim3(kHgThreads), 0, st, dy_dev, w, M, N, K,
                           (_Float16*)dx_dev);
        MDR_HIP_TRY(hipGetLastError());
    }
    if (dw_dev) {
        float* out = p.S > 1 ? (float*)(ws + p.off_dwp) : dw_dev;
        hipLaunchKernelGGL(hg_dw_kernel, dim3(K / kHgCols, N / kHgTileRows, p.S), dim3(kHgThreads), 0, st, dy_dev, x, M, N, K, out,
                           p.S > 1 ? 0 : add_old);
        MDR_HIP_TRY(hipGetLastError());
        if (p.S > 1) {
            const size_t count = (size_t)N * K;
            hipLaunchKernelGGL(hg_reduce_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const float*)out, p.S, count, dw_dev,
                               add_old);
            MDR_HIP_TRY(hipGetLastError());
        }
    }
    if (db_dev) {
        float* out = p.S > 1 ? (float*)(ws + p.off_dbp) : db_dev;
        hipLaunchKernelGGL(hg_db_kernel, dim3(N / kHgCols, p.S), dim3(kHgCols), 0, st, dy_dev, M, N, out, p.S > 1 ? 0 : add_old);
        MDR_HIP_TRY(hipGetLastError());
        if (p.S > 1) {
            hipLaunchKernelGGL(hg_reduce_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const float*)out, p.S, (size_t)N, db_dev,
                               add_old);
            MDR_HIP_TRY(hipGetLastError());
        }
    }
    return MDR_OK;
}

}  // extern "C"
