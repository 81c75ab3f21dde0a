// csrc/mdr_dropout.hip -- dropout on packed rows and the generator's test hook (include/mdr_dropout.h: mdr_dropout_threshold,
// mdr_test_dropout_bytes, mdr_dropout_rows). The mask function is csrc/mdr_dropout.h's; the attention kernels that use it live in
// csrc/mdr_attention_grad.hip.
//
// dropout_rows_kernel: one thread owns 16 consecutive elements of one row, which is one generator call (counter (col >> 4, row, 0, site)):
//   16-byte loads and stores, nothing shared between threads. Memory-bound: 2 (fp16) to 4.5 (fp32 with add16 and y16) bytes move per
//   element against one Philox call per 16.
// Rounding points: fp16 x: y = fp16(fp32(x) * m), one rounding. fp32 x: t = x (+ fp32(add16): one fp32 rounding), y = t * m (one fp32
//   rounding; exact where m = 0 and t is finite), y16 = fp16(y). m = 0 times a non-finite t is NaN: a multiplication, not a select.
#include "mdr_dropout.h"

#include "../../include/mdr_dropout.h"
#include "mdr_common.h"

namespace mdr {
namespace {

typedef _Float16 dr_half8 __attribute__((ext_vector_type(8)));
typedef float dr_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDropThreads = 256;

__global__ void __launch_bounds__(kDropThreads)
dropout_bytes_kernel(DropoutParams dp, uint32_t c2, int n0, int n1, uint4* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * kDropThreads + threadIdx.x;
    if (idx >= (size_t)n0 * n1) return;
    out[idx] = philox4x32_10((uint32_t)(idx / n1), (uint32_t)(idx % n1), c2, dp.site, dp.k0, dp.k1);
}

template <bool X16>
__global__ void __launch_bounds__(kDropThreads)
dropout_rows_kernel(const void* __restrict__ xv, const _Float16* __restrict__ add16, int M, const int* __restrict__ rows_dev, int groups, DropoutParams dp,
                    void* __restrict__ yv, _Float16* __restrict__ y16) {
    const size_t idx = (size_t)blockIdx.x * kDropThreads + threadIdx.x;
    const int valid = rows_dev ? min(*rows_dev, M) : M;
    const size_t row = idx / groups;
    if (row >= (size_t)(valid > 0 ? valid : 0)) return;
    const uint32_t grp = (uint32_t)(idx - row * groups);
    const uint4 w = philox4x32_10(grp, (uint32_t)row, 0u, dp.site, dp.k0, dp.k1);
    const uint32_t words[4] = {w.x, w.y, w.z, w.w};
    const size_t at = idx * 16;  // row * N + 16 grp
    if (X16) {
        const dr_half8* x = (const dr_half8*)((const _Float16*)xv + at);
        dr_half8* y = (dr_half8*)((_Float16*)yv + at);
        const dr_half8 v[2] = {x[0], x[1]};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            dr_half8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)((float)v[q][e] * dropout_factor(words[2 * q + (e >> 2)], e & 3, dp));
            y[q] = o;
        }
    } else {
        const dr_f32x4* x = (const dr_f32x4*)((const float*)xv + at);
        dr_f32x4* y = (dr_f32x4*)((float*)yv + at);
        dr_f32x4 v[4] = {x[0], x[1], x[2], x[3]};
        if (add16) {
            const dr_half8* a = (const dr_half8*)(add16 + at);
            const dr_half8 av[2] = {a[0], a[1]};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) v[q][e] += (float)av[q >> 1][4 * (q & 1) + e];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[q][e] *= dropout_factor(words[q], e, dp);
            y[q] = v[q];
        }
        if (y16) {
            dr_half8* h = (dr_half8*)(y16 + at);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                dr_half8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (_Float16)v[2 * q + (e >> 2)][e & 3];
                h[q] = o;
            }
        }
    }
}

}  // namespace
}  // namespace mdr

extern "C" {

int mdr_dropout_threshold(float p) { return mdr::dropout_threshold(p); }

int mdr_test_dropout_bytes(uint64_t seed, uint32_t c2, uint32_t site, int n0, int n1, void* out_dev, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_test_dropout_bytes";
    MDR_REQUIRE(out_dev, "%s: NULL pointer (out is required)", fn);
    MDR_REQUIRE(n0 >= 1 && n0 <= 65536 && n1 >= 1 && n1 <= 65536, "%s: n0=%d n1=%d out of range (1..65536)", fn, n0, n1);
    MDR_REQUIRE(aligned16({out_dev}), "%s: out must be 16-byte aligned", fn);
    MDR_ENTER_DEVICE(device);
    const size_t calls = (size_t)n0 * n1;
    hipLaunchKernelGGL(dropout_bytes_kernel, dim3((unsigned)((calls + kDropThreads - 1) / kDropThreads)), dim3(kDropThreads), 0, (hipStream_t)stream,
                       dropout_params(0, seed, site), c2, n0, n1, (uint4*)out_dev);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int mdr_dropout_rows(const void* x_dev, int x_is_fp16, const void* add16_dev, int M, const int* rows_dev, int N, int T, uint64_t seed, uint32_t site,
                     void* y_dev, void* y16_dev, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_dropout_rows";
    MDR_REQUIRE(x_dev && y_dev, "%s: NULL pointer (x and y are required)", fn);
    MDR_REQUIRE(x_is_fp16 == 0 || x_is_fp16 == 1, "%s: x_is_fp16 must be 0 or 1, got %d", fn, x_is_fp16);
    MDR_REQUIRE(!(x_is_fp16 && (add16_dev || y16_dev)), "%s: add16 and y16 go with an fp32 x only", fn);
    MDR_REQUIRE(M >= 1, "%s: M=%d out of range (>= 1)", fn, M);
    MDR_REQUIRE(N >= 16 && N % 16 == 0, "%s: N=%d must be a positive multiple of 16", fn, N);
    MDR_REQUIRE(T >= 0 && T <= 255, "%s: T=%d out of range (0..255)", fn, T);
    MDR_REQUIRE(aligned16({x_dev, add16_dev, y_dev, y16_dev}), "%s: x, add16, y and y16 must be 16-byte aligned", fn);
    const int groups = N / 16;
    const size_t blocks = ((size_t)M * groups + kDropThreads - 1) / kDropThreads;
    MDR_REQUIRE(blocks <= 0x7fffffffu, "%s: M=%d N=%d is more than one launch covers", fn, M, N);
    MDR_ENTER_DEVICE(device);
    const DropoutParams dp = dropout_params((unsigned)T, seed, site);
    if (x_is_fp16)
        hipLaunchKernelGGL(dropout_rows_kernel<true>, dim3((unsigned)blocks), dim3(kDropThreads), 0, (hipStream_t)stream, x_dev, (const _Float16*)nullptr, M,
                           rows_dev, groups, dp, y_dev, (_Float16*)nullptr);
    else
        hipLaunchKernelGGL(dropout_rows_kernel<false>, dim3((unsigned)blocks), dim3(kDropThreads), 0, (hipStream_t)stream, x_dev, (const _Float16*)add16_dev,
                           M, rows_dev, groups, dp, y_dev, (_Float16*)y16_dev);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // extern "C"
