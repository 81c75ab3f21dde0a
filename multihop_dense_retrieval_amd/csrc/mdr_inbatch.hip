// csrc/mdr_inbatch.hip -- the in-batch-negative rank step of the retriever's dev-set MRR evaluation (include/mdr_inbatch.h).
//
// One launch does both hops: grid = (ceil(B / 32) query tiles, 2 hops), 8 waves per workgroup. A workgroup stages its 32
// query rows in LDS once (mode O1: rounded to fp16 there), every wave first computes the two tiles that hold its rows'
// target columns and keeps the diagonal, then the waves sweep the 2 * ceil(B / 16) context tiles (c1 tiles, then c2 tiles,
// each section tiled from its own row 0 so that a target tile is a sweep tile) with one context fragment feeding both
// 16-query subtiles. The epilogue of a tile compares each score with the row's target score and folds an online
// log-sum-exp; nothing of the [B, 2B + 2] matrix is stored. Per-row results are combined through LDS and written by one
// lane per row.
//
// The target's score is produced by tile_mma (mdr_inbatch_tile.h), the function the sweep calls: same fragments, same K order, same
// MFMA chain, hence the same bits, and the target ties with itself exactly once (it is never counted: j < t fails).
#include "mdr_inbatch_tile.h"

namespace mdr {
namespace {

template <int MODE>
__global__ void __launch_bounds__(kIbThreads)
inbatch_rank_kernel(const float* __restrict__ q, const float* __restrict__ qsp, const float* __restrict__ ctx, const float* __restrict__ neg,
                    int B, int d, int* __restrict__ rank1, int* __restrict__ rank2, float* __restrict__ tscore1, float* __restrict__ tscore2,
                    float* __restrict__ lse1, float* __restrict__ lse2) {
    using T = typename IbElem<MODE>::T;
    extern __shared__ __attribute__((aligned(16))) char ib_lds[];
    T* qt = (T*)ib_lds;  // [kIbQT][d + PAD]
    __shared__ int p_gt[kIbWaves][kIbQT], p_tie[kIbWaves][kIbQT];
    __shared__ float p_m[kIbWaves][kIbQT], p_s[kIbWaves][kIbQT];
    __shared__ float p_ts[kIbQT], p_neg[kIbQT][2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int hop = blockIdx.y, q0 = blockIdx.x * kIbQT;
    const float* Q = hop ? qsp : q;
    const int stride = d + IbElem<MODE>::PAD;

    // ---- stage the query tile (rows past B repeat row B - 1: computed, never written) ----
    const int d4 = d >> 2;
    for (int idx = tid; idx < kIbQT * d4; idx += kIbThreads) {
        const int r = idx / d4, c4 = idx - r * d4;
        const int qr = min(q0 + r, B - 1);
        const float4 v = *(const float4*)(Q + (size_t)qr * d + 4 * c4);
        T* dst = qt + r * stride + 4 * c4;
        dst[0] = (T)v.x;
        dst[1] = (T)v.y;
        dst[2] = (T)v.z;
        dst[3] = (T)v.w;
    }
    __syncthreads();

    // ---- the two per-row negatives: 8 lanes per dot product, fp32 accumulation of the (mode O1: fp16-rounded) operands ----
    {
        const int dot = tid >> 3, sub = tid & 7;  // 64 dots = 32 rows x 2 negatives
        const int r = dot >> 1, n = dot & 1;
        const int qr = min(q0 + r, B - 1);
        const float* np = neg + ((size_t)qr * 2 + n) * d;
        const T* qp = qt + r * stride;
        float acc = 0.f;
        for (int k = 4 * sub; k < d; k += 32) {
            const float4 v = *(const float4*)(np + k);
            acc = fmaf((float)(T)v.x, (float)qp[k], acc);
            acc = fmaf((float)(T)v.y, (float)qp[k + 1], acc);
            acc = fmaf((float)(T)v.z, (float)qp[k + 2], acc);
            acc = fmaf((float)(T)v.w, (float)qp[k + 3], acc);
        }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 4);
        if (sub == 0) p_neg[r][n] = ib_score<MODE>(acc);
    }

    // ---- target scores: the diagonal of tile (q0 + 16u) / 16 of the hop's own section, by the sweep's tile code ----
    float ts[2];
    {
        const float* sec_base = ctx + (size_t)hop * B * d;
        ib_f32x4 a0, a1, b0, b1;
        const int row0 = min(q0 + c, B - 1), row1 = min(q0 + 16 + c, B - 1);
        tile_mma<MODE>(sec_base + (size_t)row0 * d, qt, stride, d, lane, a0, a1);
        tile_mma<MODE>(sec_base + (size_t)row1 * d, qt, stride, d, lane, b0, b1);
        // query column c's diagonal element is row c of the tile: register c & 3 of lane 16 * (c >> 2) + c
        const int src = 16 * (c >> 2) + c;
        ts[0] = ib_score<MODE>(__shfl(pick4(a0, c & 3), src));
        ts[1] = ib_score<MODE>(__shfl(pick4(b1, c & 3), src));
    }

    // ---- sweep ----
    int gt[2] = {0, 0}, tie[2] = {0, 0};
    float m[2] = {-INFINITY, -INFINITY}, s[2] = {0.f, 0.f};
    const int nt = (B + 15) >> 4;
    for (int tile = wave; tile < 2 * nt; tile += kIbWaves) {
        const int sec = tile >= nt ? 1 : 0;
        const int t = tile - sec * nt;
        const int arow = min(16 * t + c, B - 1);
        ib_f32x4 acc[2];
        tile_mma<MODE>(ctx + ((size_t)sec * B + arow) * d, qt, stride, d, lane, acc[0], acc[1]);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int qi = q0 + 16 * u + c;
            const int tj = hop * B + qi;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * g + r;
                const bool masked = hop == 0 && sec == 1 && row == qi;  // hop 1: the question's own bridge passage
                if (row < B && !masked) {
                    const float sc = ib_score<MODE>(acc[u][r]);
                    const int j = sec * B + row;
                    gt[u] += sc > ts[u] ? 1 : 0;
                    tie[u] += (sc == ts[u] && j < tj) ? 1 : 0;
                    lse_fold(m[u], s[u], sc);
                }
            }
        }
    }
    // lanes c, c + 16, c + 32, c + 48 hold the same query
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            gt[u] += __shfl_xor(gt[u], off);
            tie[u] += __shfl_xor(tie[u], off);
            const float m2 = __shfl_xor(m[u], off), s2 = __shfl_xor(s[u], off);
            lse_merge(m[u], s[u], m2, s2);
        }
        if (g == 0) {
            p_gt[wave][16 * u + c] = gt[u];
            p_tie[wave][16 * u + c] = tie[u];
            p_m[wave][16 * u + c] = m[u];
            p_s[wave][16 * u + c] = s[u];
            if (wave == 0) p_ts[16 * u + c] = ts[u];
        }
    }
    __syncthreads();

    // ---- one lane per row: combine the waves, add the two negatives (columns 2B, 2B + 1: never before the target), write ----
    if (tid < kIbQT && q0 + tid < B) {
        const int qi = q0 + tid;
        const float tsc = p_ts[tid];
        int n_gt = 0, n_tie = 0;
        float M = -INFINITY, S = 0.f;
        for (int w = 0; w < kIbWaves; ++w) {
            n_gt += p_gt[w][tid];
            n_tie += p_tie[w][tid];
            lse_merge(M, S, p_m[w][tid], p_s[w][tid]);
        }
        for (int n = 0; n < 2; ++n) {
            const float sc = p_neg[tid][n];
            n_gt += sc > tsc ? 1 : 0;
            lse_fold(M, S, sc);
        }
        const int rank = tsc != tsc ? 2 * B + 2 : 1 + n_gt + n_tie;
        (hop ? rank2 : rank1)[qi] = rank;
        float* tso = hop ? tscore2 : tscore1;
        float* lo = hop ? lse2 : lse1;
        if (tso) tso[qi] = tsc;
        if (lo) lo[qi] = M + logf(S);
    }
}

template <int MODE>
int launch_inbatch(const float* q, const float* qsp, const float* ctx, const float* neg, int B, int d, int* rank1, int* rank2, float* ts1,
                   float* ts2, float* lse1, float* lse2, hipStream_t stream) {
    const int lds = kIbQT * (d + IbElem<MODE>::PAD) * (int)sizeof(typename IbElem<MODE>::T);
    int rc = ensure_dynamic_lds((const void*)inbatch_rank_kernel<MODE>, kIbQT * (kIbMaxD + IbElem<MODE>::PAD) * (int)sizeof(typename IbElem<MODE>::T));
    if (rc != MDR_OK) return rc;
    const dim3 grid((unsigned)((B + kIbQT - 1) / kIbQT), 2);
    hipLaunchKernelGGL(inbatch_rank_kernel<MODE>, grid, dim3(kIbThreads), lds, stream, q, qsp, ctx, neg, B, d, rank1, rank2, ts1, ts2, lse1, lse2);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

bool ib_shape_ok(int B, int d, int mode) {
    return B >= 1 && B <= (1 << 24) && d >= 32 && d <= kIbMaxD && d % 32 == 0 && (mode == MDR_INBATCH_F32 || mode == MDR_INBATCH_O1);
}

}  // namespace
}  // namespace mdr

extern "C" {

size_t mdr_inbatch_workspace_bytes(int B, int d, int mode) {
    (void)B, (void)d, (void)mode;
    return 0;  // the partial results of a row tile live in LDS
}

int mdr_inbatch_rank(const float* q_dev, const float* qsp_dev, const float* ctx_dev, const float* neg_dev, int B, int d, int mode,
                     int32_t* rank1_dev, int32_t* rank2_dev, float* tscore1_dev, float* tscore2_dev, float* lse1_dev, float* lse2_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream) {
    using namespace mdr;
    (void)workspace_dev, (void)workspace_bytes;
    MDR_REQUIRE(B >= 1, "mdr_inbatch_rank: B = %d, need B >= 1", B);
    MDR_REQUIRE(mode == MDR_INBATCH_F32 || mode == MDR_INBATCH_O1, "mdr_inbatch_rank: unknown mode %d", mode);
    MDR_REQUIRE(ib_shape_ok(B, d, mode), "mdr_inbatch_rank: B = %d, d = %d unsupported (d a multiple of 32 in [32, %d], B <= 2^24)", B, d, kIbMaxD);
    MDR_REQUIRE(q_dev && qsp_dev && ctx_dev && neg_dev, "mdr_inbatch_rank: q, qsp, ctx and neg must not be NULL");
    MDR_REQUIRE(rank1_dev && rank2_dev, "mdr_inbatch_rank: rank1 and rank2 must not be NULL");
    MDR_REQUIRE((((uintptr_t)q_dev | (uintptr_t)qsp_dev | (uintptr_t)ctx_dev | (uintptr_t)neg_dev) & 15) == 0,
                "mdr_inbatch_rank: q, qsp, ctx and neg must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (mode == MDR_INBATCH_O1)
        return launch_inbatch<MDR_INBATCH_O1>(q_dev, qsp_dev, ctx_dev, neg_dev, B, d, rank1_dev, rank2_dev, tscore1_dev, tscore2_dev, lse1_dev, lse2_dev, st);
    return launch_inbatch<MDR_INBATCH_F32>(q_dev, qsp_dev, ctx_dev, neg_dev, B, d, rank1_dev, rank2_dev, tscore1_dev, tscore2_dev, lse1_dev, lse2_dev, st);
}

}  // extern "C"
