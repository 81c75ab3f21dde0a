// csrc/mdr_reader_select.hip -- the reader's chain selection (include/mdr_reader_select.h): per question and per combination factor the
// item that predict()'s sequence of in-place stable sorts leaves on top, plus the first item with the largest rank score.
//
// One wave per question, four waves per workgroup. A question has at most a few hundred chains (the README's dev file: 50), so its two
// fp16 score rows sit in L1 / L2 after the first pass and the kernel makes one pass per factor instead of keeping sixteen running
// winners per lane: a pass holds ONE candidate (two fp16 patterns and an index) per lane, nothing is indexed dynamically and nothing
// spills. Lanes stride over the segment in increasing index order; the wave's result is a butterfly of __shfl_xor steps under the same
// comparator, which is a strict total order over the items (key tuples compare lexicographically, equal tuples by index), so the result
// does not depend on how the segment was split over the lanes. No LDS, no atomics.
//
// Rounding. A key is fl(fl(lambda * r) + fl(one_minus * s)) in fp64 from the exactly widened fp16 scores: two products and one sum, each
// rounded on its own (the pragma below keeps the compiler from contracting them), which is what Python computes for
// `lambda_ * x["rank_score"] + (1 - lambda_) * x["span_score"]`. Keys are recomputed whenever two items are compared; none is stored.
// Questions with a non-finite score never reach a key: they are flagged in the first pass and left to the host.
#include "mdr_common.h"
#include "../../include/mdr_reader_select.h"

#pragma clang fp contract(off)

namespace mdr {
namespace {

constexpr int kSelWave = 64;
constexpr int kSelWaves = 4;  // questions per workgroup

struct SelectFactors {
    double lam[MDR_READER_SELECT_MAX_LAMBDAS];
    double om[MDR_READER_SELECT_MAX_LAMBDAS];
};

struct Cand {
    int idx;         // item index, -1: none
    unsigned bits;   // rank16 << 16 | span16
};

__device__ inline double widen(unsigned bits16) { return (double)__builtin_bit_cast(_Float16, (unsigned short)bits16); }
__device__ inline bool non_finite(unsigned bits16) { return (bits16 & 0x7C00u) == 0x7C00u; }

// a goes before b in the order the sorts for factors 0 .. k leave: the larger (key_k, ..., key_0), then the lower index
__device__ inline bool before(const Cand& a, const Cand& b, int k, const SelectFactors& f) {
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    const double ra = widen(a.bits >> 16), sa = widen(a.bits & 0xFFFFu), rb = widen(b.bits >> 16), sb = widen(b.bits & 0xFFFFu);
    for (int j = k; j >= 0; --j) {
        const double pa = f.lam[j] * ra, qa = f.om[j] * sa, pb = f.lam[j] * rb, qb = f.om[j] * sb;
        const double ka = pa + qa, kb = pb + qb;
        if (ka > kb) return true;
        if (ka < kb) return false;
    }
    return a.idx < b.idx;
}

// a goes before b under the rank score alone
__device__ inline bool rank_before(const Cand& a, const Cand& b) {
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    const double ra = widen(a.bits >> 16), rb = widen(b.bits >> 16);
    if (ra > rb) return true;
    if (ra < rb) return false;
    return a.idx < b.idx;
}

__device__ inline Cand from_lane(const Cand& c, int mask) {
    Cand o;
    o.idx = __shfl_xor(c.idx, mask, kSelWave);
    o.bits = (unsigned)__shfl_xor((int)c.bits, mask, kSelWave);
    return o;
}

__global__ __launch_bounds__(kSelWave* kSelWaves) void reader_select_kernel(const unsigned short* __restrict__ rank16,
                                                                            const unsigned short* __restrict__ span16,
                                                                            const long long* __restrict__ q_offsets, int n_q, SelectFactors f,
                                                                            int n_lambda, int* __restrict__ winners, int* __restrict__ rank_top,
                                                                            int* __restrict__ flags) {
    const int lane = threadIdx.x & (kSelWave - 1);
    const int q = blockIdx.x * kSelWaves + (threadIdx.x / kSelWave);
    if (q >= n_q) return;  // the whole wave
    const long long lo = q_offsets[q], hi = q_offsets[q + 1];
    int* const win = winners + (long long)q * n_lambda;

    // pass 0: non-finite scores and the top rank score
    bool bad = false;
    Cand best{-1, 0u};
    for (long long i = lo + lane; i < hi; i += kSelWave) {
        const unsigned r = rank16[i], s = span16[i];
        bad = bad || non_finite(r) || non_finite(s);
        const Cand cur{(int)i, r << 16 | s};
        if (rank_before(cur, best)) best = cur;
    }
    if (__ballot(bad) != 0) {  // keys would be NaN: the host sorts this question
        if (lane < n_lambda) win[lane] = -1;
        if (lane == 0) {
            rank_top[q] = -1;
            flags[q] = 1;
        }
        return;
    }
    for (int m = kSelWave / 2; m >= 1; m >>= 1) {
        const Cand other = from_lane(best, m);
        if (rank_before(other, best)) best = other;
    }
    if (lane == 0) {
        rank_top[q] = best.idx;
        flags[q] = 0;
    }

    // one pass per factor
    for (int k = 0; k < n_lambda; ++k) {
        best = Cand{-1, 0u};
        for (long long i = lo + lane; i < hi; i += kSelWave) {
            const Cand cur{(int)i, (unsigned)rank16[i] << 16 | (unsigned)span16[i]};
            if (before(cur, best, k, f)) best = cur;
        }
        for (int m = kSelWave / 2; m >= 1; m >>= 1) {
            const Cand other = from_lane(best, m);
            if (before(other, best, k, f)) best = other;
        }
        if (lane == 0) win[k] = best.idx;
    }
}

}  // namespace
}  // namespace mdr

extern "C" int mdr_reader_select(const uint16_t* rank16_dev, const uint16_t* span16_dev, const int64_t* q_offsets_dev, int n_q, const double* lambdas,
                                 const double* one_minus, int n_lambda, int32_t* winners_dev, int32_t* rank_top_dev, int32_t* flags_dev, int device,
                                 void* stream) {
    using namespace mdr;
    const char* fn = "mdr_reader_select";
    MDR_REQUIRE(n_q >= 0, "%s: n_q=%d must not be negative", fn, n_q);
    MDR_REQUIRE(n_lambda >= 1 && n_lambda <= MDR_READER_SELECT_MAX_LAMBDAS, "%s: n_lambda=%d must lie in 1 .. %d", fn, n_lambda,
                MDR_READER_SELECT_MAX_LAMBDAS);
    if (n_q == 0) return MDR_OK;
    MDR_REQUIRE(rank16_dev && span16_dev && q_offsets_dev && lambdas && one_minus && winners_dev && rank_top_dev && flags_dev, "%s: NULL pointer", fn);
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    SelectFactors f{};
    for (int k = 0; k < n_lambda; ++k) {
        f.lam[k] = lambdas[k];
        f.om[k] = one_minus[k];
    }
    const unsigned blocks = ((unsigned)n_q + kSelWaves - 1) / kSelWaves;
    hipLaunchKernelGGL(reader_select_kernel, dim3(blocks), dim3(kSelWave * kSelWaves), 0, (hipStream_t)stream, (const unsigned short*)rank16_dev,
                       (const unsigned short*)span16_dev, (const long long*)q_offsets_dev, n_q, f, n_lambda, (int*)winners_dev, (int*)rank_top_dev,
                       (int*)flags_dev);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}
