// csrc/mdr_rank_sum.hip -- the ordered gradient sum of multi-rank training (include/mdr_rank_sum.h): out[i] = the fp32 sum over the rows
// of recv at column i, strictly left to right in rank order, the accumulator starting at row 0.
//
// A streaming kernel: N reads and one write per element, no reuse, no LDS. Thread t of a 256-thread workgroup owns one group of four
// columns at a time (one 16-byte load per row, one 16-byte store), the grid is capped at 2048 workgroups and strides over the groups.
// The row count is a template argument, so the N loads of a group are all issued before the first addition waits for one (N <= 16: at most
// 64 VGPRs of loads in flight). The n % 4 columns behind the last whole group are read and written element by element, so nothing behind
// out[n) is written and nothing of a row's padding n .. stride reaches a result. Rows start at multiples of `stride`, stride % 4 == 0 and
// recv is 16-byte aligned: every vector access is aligned.
//
// Rounding. One fp32 addition per row behind the first, in rank order, none contracted (the pragma below) and none reassociated: numpy
// float32 adding one row after another gives the same bits (dist.rank_sum_host). With one row the value is moved, not added to 0: its bits
// survive, a NaN's payload and -0.0 included.
#include <algorithm>

#include "mdr_common.h"
#include "../../include/mdr_rank_sum.h"

#pragma clang fp contract(off)

namespace mdr {
namespace {

constexpr int kRsThreads = 256;
constexpr int kRsMaxGrid = 2048;

template <int N>
__global__ __launch_bounds__(kRsThreads) void rank_sum_kernel(const float* __restrict__ recv, int64_t n, int64_t stride, float* __restrict__ out) {
    const int64_t groups = n >> 2;
    const int64_t step = (int64_t)gridDim.x * kRsThreads;
    const int64_t first = (int64_t)blockIdx.x * kRsThreads + threadIdx.x;
    for (int64_t g = first; g < groups; g += step) {
        float4 v[N];
#pragma unroll
        for (int r = 0; r < N; ++r) v[r] = *reinterpret_cast<const float4*>(recv + r * stride + g * 4);
        float4 acc = v[0];
#pragma unroll
        for (int r = 1; r < N; ++r) {
            acc.x = acc.x + v[r].x;
            acc.y = acc.y + v[r].y;
            acc.z = acc.z + v[r].z;
            acc.w = acc.w + v[r].w;
        }
        *reinterpret_cast<float4*>(out + g * 4) = acc;
    }
    const int64_t i = groups * 4 + first;  // the scalar tail: at most three columns, the first threads of the grid
    if (i < n) {
        float acc = recv[i];
#pragma unroll
        for (int r = 1; r < N; ++r) acc = acc + recv[r * stride + i];
        out[i] = acc;
    }
}

template <int N>
int launch_rank_sum(const float* recv, int64_t n, int64_t stride, float* out, hipStream_t st) {
    const int64_t blocks = std::max<int64_t>(1, ((n >> 2) + kRsThreads - 1) / kRsThreads);
    hipLaunchKernelGGL(rank_sum_kernel<N>, dim3((unsigned)std::min<int64_t>(blocks, kRsMaxGrid)), dim3(kRsThreads), 0, st, recv, n, stride, out);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // namespace
}  // namespace mdr

extern "C" {

int mdr_rank_sum(const float* recv, int n_ranks, int64_t n, int64_t stride, float* out, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_rank_sum";
    MDR_REQUIRE(recv && out, "%s: NULL pointer (recv and out are required)", fn);
    MDR_REQUIRE(n_ranks >= 1 && n_ranks <= MDR_RANK_SUM_MAX_RANKS, "%s: n_ranks=%d must lie in 1 .. %d", fn, n_ranks, MDR_RANK_SUM_MAX_RANKS);
    MDR_REQUIRE(n >= 1, "%s: n=%lld must be at least 1", fn, (long long)n);
    MDR_REQUIRE(stride >= n && stride % 4 == 0 && stride <= INT64_MAX / (MDR_RANK_SUM_MAX_RANKS * 4),
                "%s: stride=%lld must be a multiple of 4, at least n=%lld", fn, (long long)stride, (long long)n);
    MDR_REQUIRE(aligned16({recv, out}), "%s: recv and out must be 16-byte aligned", fn);
    const float* recv_end = recv + (n_ranks - 1) * stride + n;  // behind the last column any row is read at
    MDR_REQUIRE((uintptr_t)(out + n) <= (uintptr_t)recv || (uintptr_t)recv_end <= (uintptr_t)out, "%s: out[0 .. n) overlaps the rows of recv", fn);
    hipStream_t st = (hipStream_t)stream;
    switch (n_ranks) {
#define MDR_RS_CASE(N) \
    case N:            \
        return launch_rank_sum<N>(recv, n, stride, out, st);
        MDR_RS_CASE(1) MDR_RS_CASE(2) MDR_RS_CASE(3) MDR_RS_CASE(4) MDR_RS_CASE(5) MDR_RS_CASE(6) MDR_RS_CASE(7) MDR_RS_CASE(8)
        MDR_RS_CASE(9) MDR_RS_CASE(10) MDR_RS_CASE(11) MDR_RS_CASE(12) MDR_RS_CASE(13) MDR_RS_CASE(14) MDR_RS_CASE(15) MDR_RS_CASE(16)
#undef MDR_RS_CASE
    }
    return set_error(MDR_E_INVALID, "%s: n_ranks=%d", fn, n_ranks);
}

}  // extern "C"
