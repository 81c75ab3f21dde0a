// csrc/mdr_linear_grad.inl -- the backward of a Linear of the trunk on packed rows (include/mdr_linear_grad.h: mdr_linear_backward):
//     Y[M, N] = act(X[M, K] W[N, K]^T + b[N]):   dZ = dY o gelu'(u) (or dY)   dX = dZ W   dW = dZ^T X   db = column sums of dZ
// Included at the end of mdr_encoder.hip (not a translation unit of its own), so that dX can go through launch_gemm.
//
// lg_gelu_grad_kernel   dZ = fp16(dY * gelu'(u)), one 16-byte piece per thread; rows at or behind the valid count are written as zeros.
// lg_transpose_kernel   W[N, K] -> W^T[K, N] through a 64 x 64 LDS tile. dX = dZ W is then the encoder's own forward GEMM
//                       (launch_gemm<EPI_BIAS_F16>, A = dZ, "W" = W^T, a zero bias from the workspace, the same m_dev): no second dense GEMM.
// lg_wgrad_kernel       dW = dZ^T X, the contraction over the token index, which is the ROW index of both operands. A workgroup of four
//                       waves owns one 128 (n) x 128 (k) tile of dW, a wave a 64 x 64 quarter of it (N and K are multiples of 64 only:
//                       a quarter past N or K computes on zero-filled columns and stores nothing), and one chunk of the token rows. It
//                       stages slabs of 64 rows of dZ[rows, n-tile] and X[rows, k-tile] row-major in LDS (register staging: the next slab's
//                       global loads are in flight while the MFMAs of this one run; 256-byte rows, 16-byte pieces XOR-swizzled so that
//                       the transposed reads are conflict-free) and reads BOTH MFMA operands with ds_read_b64_tr_b16: lane a of a 16-lane
//                       group addresses row a >> 2, columns 4 (a & 3) .. of a [4 rows][16 columns] block and receives column a. k-slot
//                       (g, j) of v_mfma_f32_16x16x32_f16 is token row 32 step + 8 g + j in both operands. Rows at or behind the valid
//                       count are zero-filled while staging. With S > 1 chunks the tile goes to the fp32 workspace [S][N][K].
// lg_colsum_kernel      db partial of one chunk and 64 columns: 32 row groups x 8 pieces, each thread an fp32 sum over its rows in order,
//                       then the 32 partial sums in order. A kernel of its own rather than a job of the first k-tile's workgroups: the
//                       MFMA kernel keeps one role per workgroup and no column-wise LDS pass, and db re-reads only M x N fp16.
// lg_reduce_kernel      out = partial[0] + partial[1] + ... + partial[S - 1] (in this order), then + the old value if `accumulate`.
// Every output element has one owner and one summation order: no atomics, and two runs give the same bits.
//
// Rounding points (tests/linear_grad_ref.py derives its bound from this list):
//   1. x, w, dy and u are fp16: exact operands. A product of two fp16 is exact in fp32, but an MFMA adds the products of one instruction
//      aligned to their largest exponent FIELD with 24 bits kept below it, and a subnormal or zero operand carries the field 2^-14 whatever
//      its value: a sum of subnormal x normal products alone (FFN2's dW over a few CLS rows, a GELU-output column deep in the negative tail)
//      loses up to ten bits. Nothing to do about it here; the bound has a term for it.
//   2. gelu'(u) = Phi(u) + u phi(u) in fp32. Phi from the forward's tail polynomial (gelu_erf2 of mdr_encoder_gemm.inl, max |Phi error|
//      2.1e-7) evaluated at min(|u|, 16) -- the polynomial is fitted on [0, 6] and turns around near 23.5, and Phi(-16) is 0 in fp32 --
//      phi(u) = exp2(-u^2 log2(e) / 2) / sqrt(2 pi) from one v_exp_f32. dZ = fp16(fp32(dy) * gelu'(u)): one fp16 rounding.
//   3. dX: fp32 MFMA sums of N exact products (the forward GEMM), + 0.0f (the zero bias), rounded to fp16 once.
//   4. dW: fp32 MFMA sums over the rows of a chunk in slab order, the chunks added in order in fp32, then the old value: no further rounding.
//   5. db: fp32 sums in the fixed order above, chunks in order, then the old value: no further rounding.

#include "../../include/mdr_linear_grad.h"

namespace {

typedef __fp16 lg_fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

constexpr int kLgSlab = 64;            // token rows per staged slab: two MFMA k-steps of 32
constexpr int kLgTile = 128;           // dW tile edge; a wave owns a 64 x 64 quarter
constexpr int kLgThreads = 256;
constexpr int kLgImage = kLgSlab * 256;  // bytes of one staged image: 64 rows of 128 fp16
constexpr int kLgPieces = kLgSlab * 16 / kLgThreads;  // 16-byte pieces per thread per image
constexpr int kLgTargetWgs = 512;      // workgroups the split aims at (two per CU of a 256-CU part); a constant, NOT the device's count

// byte offset of 16-byte piece ch (0..15) of row `row` in an image of 256-byte rows
__device__ __forceinline__ int lg_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// rows row0 .. row0 + 63 (below row_end) x columns col0 .. col0 + 127 (below ncols) of src[., ld] into registers, everything else zero
__device__ __forceinline__ void lg_load(const _Float16* __restrict__ src, int ld, int row0, int row_end, int col0, int ncols, int tid,
                                        half8 (&v)[kLgPieces]) {
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < kLgPieces; ++u) {
        const int p = tid + u * kLgThreads, row = row0 + (p >> 4), col = col0 + (p & 15) * 8;
        v[u] = zero8;
        if (row < row_end && col < ncols) v[u] = *(const half8*)(src + (size_t)row * ld + col);
    }
}

__device__ __forceinline__ void lg_put(char* img, int tid, const half8 (&v)[kLgPieces]) {
#pragma unroll
    for (int u = 0; u < kLgPieces; ++u) {
        const int p = tid + u * kLgThreads;
        *(half8*)(img + lg_off(p >> 4, p & 15)) = v[u];
    }
}

__device__ __forceinline__ half8 lg_tr_pair(const char* lo_p, const char* hi_p) {
    const lg_fp16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) lg_fp16x4*)lo_p);
    const lg_fp16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) lg_fp16x4*)hi_p);
    return (half8){(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3], (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2], (_Float16)hi[3]};
}

// grid (n-tiles * k-tiles, S). out: dw itself (S == 1) or the partials [S][N][K].
__global__ void __launch_bounds__(kLgThreads)
lg_wgrad_kernel(const _Float16* __restrict__ dy, const _Float16* __restrict__ x, int M_cap, const int* __restrict__ M_dev, int N, int K,
                int rows_per_chunk, float* __restrict__ out, int add_old) {
    __shared__ __attribute__((aligned(256))) char img_dy[kLgImage];
    __shared__ __attribute__((aligned(256))) char img_x[kLgImage];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, lr = lane & 15;
    const int M = M_dev ? min(max(*M_dev, 0), M_cap) : M_cap;
    const int tiles_k = (K + kLgTile - 1) / kLgTile;
    const int n0 = ((int)blockIdx.x / tiles_k) * kLgTile, k0 = ((int)blockIdx.x % tiles_k) * kLgTile;
    const int chunk = blockIdx.y;
    const int row_begin = chunk * rows_per_chunk;
    const int row_end = min(row_begin + rows_per_chunk, M);  // (row_end <= row_begin: a chunk behind the valid rows stores zeros)
    const int wn = wave >> 1, wk = wave & 1;

    // transposed reads: the group's block for k-step half `h` is rows 8 g + 4 h .. + 3; this lane addresses row q of it, 4 columns at 4 p
    const int q = lr >> 2, p = lr & 3;
    int off_dy[4][2], off_x[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = 8 * g + 4 * h + q;
            off_dy[t][h] = lg_off(row, wn * 8 + 2 * t + (p >> 1)) + 8 * (p & 1);
            off_x[t][h] = lg_off(row, wk * 8 + 2 * t + (p >> 1)) + 8 * (p & 1);
        }

    f32x4 acc[4][4];  // [dy column tile tb][x column tile ta]: dW[n0 + 64 wn + 16 tb + lr][k0 + 64 wk + 16 ta + 4 g + r]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    half8 vdy[kLgPieces], vx[kLgPieces];
    lg_load(dy, N, row_begin, row_end, n0, N, tid, vdy);
    lg_load(x, K, row_begin, row_end, k0, K, tid, vx);
    for (int r0 = row_begin; r0 < row_end; r0 += kLgSlab) {
        __syncthreads();  // the previous slab's reads are done
        lg_put(img_dy, tid, vdy);
        lg_put(img_x, tid, vx);
        __syncthreads();
        if (r0 + kLgSlab < row_end) {
            lg_load(dy, N, r0 + kLgSlab, row_end, n0, N, tid, vdy);
            lg_load(x, K, r0 + kLgSlab, row_end, k0, K, tid, vx);
        }
#pragma unroll
        for (int step = 0; step < kLgSlab / 32; ++step) {
            half8 fdy[4], fx[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                fdy[t] = lg_tr_pair(img_dy + step * 32 * 256 + off_dy[t][0], img_dy + step * 32 * 256 + off_dy[t][1]);
                fx[t] = lg_tr_pair(img_x + step * 32 * 256 + off_x[t][0], img_x + step * 32 * 256 + off_x[t][1]);
            }
#pragma unroll
            for (int tb = 0; tb < 4; ++tb)
#pragma unroll
                for (int ta = 0; ta < 4; ++ta) acc[tb][ta] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fx[ta], fdy[tb], acc[tb][ta], 0, 0, 0);
        }
    }
    // the stores sit behind a branch, where hipcc's hazard recogniser does not look for the distance a VALU read of an MFMA result needs
    asm volatile("s_nop 7\n\ts_nop 7" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[0][3]), "+v"(acc[1][0]), "+v"(acc[1][1]),
                 "+v"(acc[1][2]), "+v"(acc[1][3]), "+v"(acc[2][0]), "+v"(acc[2][1]), "+v"(acc[2][2]), "+v"(acc[2][3]), "+v"(acc[3][0]),
                 "+v"(acc[3][1]), "+v"(acc[3][2]), "+v"(acc[3][3]));
    const int nb = n0 + 64 * wn, kb = k0 + 64 * wk;
    if (nb >= N || kb >= K) return;  // a quarter past the matrix (N, K are multiples of 64: a quarter is inside or outside as a whole)
    float* o = out + (size_t)chunk * (size_t)N * (size_t)K;
#pragma unroll
    for (int tb = 0; tb < 4; ++tb)
#pragma unroll
        for (int ta = 0; ta < 4; ++ta) {
            float* ptr = o + (size_t)(nb + 16 * tb + lr) * K + kb + 16 * ta + 4 * g;
            f32x4 v = acc[tb][ta];
            if (add_old) v += *(const f32x4*)ptr;
            *(f32x4*)ptr = v;
        }
}

// grid (N / 64, S). out: db itself (S == 1) or the partials [S][N].
__global__ void __launch_bounds__(kLgThreads)
lg_colsum_kernel(const _Float16* __restrict__ dy, int M_cap, const int* __restrict__ M_dev, int N, int rows_per_chunk, float* __restrict__ out,
                 int add_old) {
    __shared__ float red[32][64];
    const int tid = threadIdx.x, rg = tid >> 3, cc = tid & 7;
    const int M = M_dev ? min(max(*M_dev, 0), M_cap) : M_cap;
    const int n0 = blockIdx.x * 64, chunk = blockIdx.y;
    const int row_begin = chunk * rows_per_chunk, row_end = min(row_begin + rows_per_chunk, M);
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = row_begin + rg; r < row_end; r += 32) {
        const half8 v = *(const half8*)(dy + (size_t)r * N + n0 + cc * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += (float)v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[rg][cc * 8 + j] = s[j];
    __syncthreads();
    if (tid < 64) {
        float t = red[0][tid];
        for (int i = 1; i < 32; ++i) t += red[i][tid];
        float* ptr = out + (size_t)chunk * N + n0 + tid;
        if (add_old) t += *ptr;
        *ptr = t;
    }
}

// out[i] = part[0][i] + part[1][i] + ... + part[S - 1][i] (+ out[i] last); count is a multiple of 4
__global__ void __launch_bounds__(256)
lg_reduce_kernel(const float* __restrict__ part, int S, size_t count, float* __restrict__ out, int add_old) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= count) return;
    f32x4 t = *(const f32x4*)(part + i);
    for (int s = 1; s < S; ++s) t += *(const f32x4*)(part + (size_t)s * count + i);
    if (add_old) t += *(const f32x4*)(out + i);
    *(f32x4*)(out + i) = t;
}

// grid (K / 64, N / 64): wt[k][n] = w[n][k]
__global__ void __launch_bounds__(256)
lg_transpose_kernel(const _Float16* __restrict__ w, int N, int K, _Float16* __restrict__ wt) {
    __shared__ _Float16 tile[64][72];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int p = tid + u * 256, r = p >> 3, c = (p & 7) * 8;
        *(half8*)(&tile[r][c]) = *(const half8*)(w + (size_t)(n0 + r) * K + k0 + c);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int p = tid + u * 256, r = p >> 3, c = (p & 7) * 8;  // output row k0 + r, columns n0 + c ..
        half8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = tile[c + j][r];
        *(half8*)(wt + (size_t)(k0 + r) * N + n0 + c) = v;
    }
}

// Phi(u) - 1/2 from the forward's tail polynomial, for a pair of values: the forward's own helper (mdr_encoder_gemm.inl), clamp included
__device__ inline f32x2 lg_phi_m_half2(f32x2 u) { return gelu_phi_m_half2(u); }

// one 16-byte piece per thread: dz = fp16(dy * (Phi(u) + u phi(u))); rows at or behind the valid count: zeros, nothing read
__global__ void __launch_bounds__(256)
lg_gelu_grad_kernel(const _Float16* __restrict__ dy, const _Float16* __restrict__ pre, int M_cap, const int* __restrict__ M_dev, int N,
                    _Float16* __restrict__ dz) {
    const size_t piece = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per_row = (size_t)N / 8;
    if (piece >= (size_t)M_cap * per_row) return;
    const int M = M_dev ? min(max(*M_dev, 0), M_cap) : M_cap;
    const int row = (int)(piece / per_row);
    half8 o = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < M) {
        const half8 d = *(const half8*)(dy + piece * 8), u8 = *(const half8*)(pre + piece * 8);
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const f32x2 u = {(float)u8[j], (float)u8[j + 1]};
            const f32x2 s = lg_phi_m_half2(u);
            f32x2 dens;  // phi(u)
            dens[0] = __builtin_amdgcn_exp2f(u[0] * u[0] * -0.72134752044448170f) * 0.3989422804014327f;
            dens[1] = __builtin_amdgcn_exp2f(u[1] * u[1] * -0.72134752044448170f) * 0.3989422804014327f;
            const f32x2 gp = (s + 0.5f) + u * dens;
            o[j] = (_Float16)((float)d[j] * gp[0]);
            o[j + 1] = (_Float16)((float)d[j + 1] * gp[1]);
        }
    }
    *(half8*)(dz + piece * 8) = o;
}

struct LgPlan {
    int S = 0, rows_per_chunk = 0;
    size_t off_dz = 0, off_wt = 0, off_bias = 0, off_dwp = 0, off_dbp = 0, bytes = 0;
};

bool lg_shape_ok(int M, int N, int K) { return M >= 1 && N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0; }

// the split: a function of (M, N, K) alone
int lg_chunks(int M, int N, int K, int* rows_per_chunk) {
    const long long tiles = (long long)((N + kLgTile - 1) / kLgTile) * ((K + kLgTile - 1) / kLgTile);
    const long long slabs = ((long long)M + kLgSlab - 1) / kLgSlab;
    long long want = (kLgTargetWgs + tiles - 1) / tiles;
    want = std::max(1ll, std::min(want, slabs));
    const long long per = (slabs + want - 1) / want;
    if (rows_per_chunk) *rows_per_chunk = (int)(per * kLgSlab);
    return (int)((slabs + per - 1) / per);
}

LgPlan lg_plan(int M, int N, int K, int want) {
    LgPlan p;
    p.S = lg_chunks(M, N, K, &p.rows_per_chunk);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align_up(bytes, 256); return o; };
    if (want & MDR_LINEAR_WANT_PRE) p.off_dz = take((size_t)M * N * 2);
    if (want & MDR_LINEAR_WANT_DX) {
        p.off_wt = take((size_t)N * K * 2);
        p.off_bias = take((size_t)K * 4);
    }
    if ((want & MDR_LINEAR_WANT_DW) && p.S > 1) p.off_dwp = take((size_t)p.S * N * K * 4);
    if ((want & MDR_LINEAR_WANT_DB) && p.S > 1) p.off_dbp = take((size_t)p.S * N * 4);
    p.bytes = at;
    return p;
}

}  // namespace

extern "C" {

int mdr_linear_backward_chunks(int M, int N, int K, int* rows_per_chunk) {
    if (!lg_shape_ok(M, N, K)) {
        if (rows_per_chunk) *rows_per_chunk = 0;
        return 0;
    }
    return lg_chunks(M, N, K, rows_per_chunk);
}

size_t mdr_linear_backward_workspace_bytes(int M, int N, int K, int want) {
    if (!lg_shape_ok(M, N, K)) return 0;
    return lg_plan(M, N, K, want).bytes;
}

int mdr_linear_backward(const void* x_dev, const void* w_dev, const void* dy_dev, const void* pre_dev, int M, const int* m_dev, int N, int K,
                        void* dx_dev, float* dw_dev, float* db_dev, int accumulate, void* workspace_dev, size_t workspace_bytes, int device,
                        void* stream) {
    MDR_REQUIRE(x_dev && w_dev && dy_dev, "NULL pointer: x, w and dy are required");
    MDR_REQUIRE(dx_dev || dw_dev || db_dev, "nothing to compute: dx, dw and db are all NULL");
    MDR_REQUIRE(M >= 1, "M=%d must be at least 1", M);
    MDR_REQUIRE(N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0, "bad Linear shape N=%d K=%d (positive multiples of 64)", N, K);
    MDR_REQUIRE(aligned16({x_dev, w_dev, dy_dev, pre_dev, dx_dev, dw_dev, db_dev, workspace_dev}), "pointers must be 16-byte aligned");
    const int want = (dx_dev ? MDR_LINEAR_WANT_DX : 0) | (dw_dev ? MDR_LINEAR_WANT_DW : 0) | (db_dev ? MDR_LINEAR_WANT_DB : 0) |
                     (pre_dev ? MDR_LINEAR_WANT_PRE : 0);
    const LgPlan p = lg_plan(M, N, K, want);
    MDR_REQUIRE_WORKSPACE("mdr_linear_backward", workspace_dev, workspace_bytes, p.bytes, "mdr_linear_backward_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace_dev;
    const _Float16* x = (const _Float16*)x_dev;
    const _Float16* w = (const _Float16*)w_dev;
    const _Float16* dz = (const _Float16*)dy_dev;
    const int add_old = accumulate ? 1 : 0;

    if (pre_dev) {
        _Float16* dzw = (_Float16*)(ws + p.off_dz);
        const size_t pieces = (size_t)M * (N / 8);
        hipLaunchKernelGGL(lg_gelu_grad_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, (const _Float16*)dy_dev,
                           (const _Float16*)pre_dev, M, m_dev, N, dzw);
        MDR_HIP_TRY(hipGetLastError());
        dz = dzw;
    }
    if (dx_dev) {
        _Float16* wt = (_Float16*)(ws + p.off_wt);
        float* zero_bias = (float*)(ws + p.off_bias);
        MDR_HIP_TRY(hipMemsetAsync(zero_bias, 0, (size_t)K * 4, st));
        hipLaunchKernelGGL(lg_transpose_kernel, dim3(K / 64, N / 64), dim3(256), 0, st, w, N, K, wt);
        MDR_HIP_TRY(hipGetLastError());
        const int ncu = device_cu_count(device);
        if (int rc = launch_gemm<EPI_BIAS_F16>(dz, N, wt, zero_bias, M, m_dev, K, N, dx_dev, K, nullptr, 0, M, ncu, st)) return rc;
    }
    if (dw_dev) {
        const unsigned tiles = (unsigned)(((N + kLgTile - 1) / kLgTile) * ((K + kLgTile - 1) / kLgTile));
        float* out = p.S > 1 ? (float*)(ws + p.off_dwp) : dw_dev;
        hipLaunchKernelGGL(lg_wgrad_kernel, dim3(tiles, p.S), dim3(kLgThreads), 0, st, dz, x, M, m_dev, N, K, p.rows_per_chunk, out,
                           p.S > 1 ? 0 : add_old);
        MDR_HIP_TRY(hipGetLastError());
        if (p.S > 1) {
            const size_t count = (size_t)N * K;
            hipLaunchKernelGGL(lg_reduce_kernel, dim3((unsigned)((count / 4 + 255) / 256)), dim3(256), 0, st, (const float*)out, p.S, count, dw_dev,
                               add_old);
            MDR_HIP_TRY(hipGetLastError());
        }
    }
    if (db_dev) {
        float* out = p.S > 1 ? (float*)(ws + p.off_dbp) : db_dev;
        hipLaunchKernelGGL(lg_colsum_kernel, dim3(N / 64, p.S), dim3(kLgThreads), 0, st, dz, M, m_dev, N, p.rows_per_chunk, out,
                           p.S > 1 ? 0 : add_old);
        MDR_HIP_TRY(hipGetLastError());
        if (p.S > 1) {
            hipLaunchKernelGGL(lg_reduce_kernel, dim3((unsigned)((N / 4 + 255) / 256)), dim3(256), 0, st, (const float*)out, p.S, (size_t)N, db_dev,
                               add_old);
            MDR_HIP_TRY(hipGetLastError());
        }
    }
    return MDR_OK;
}

}  // extern "C"
