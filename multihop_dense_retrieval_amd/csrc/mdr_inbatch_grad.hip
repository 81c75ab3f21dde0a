// csrc/mdr_inbatch_grad.hip -- the in-batch retrieval loss over 2B + 2 + K columns (the batch's passages, the row's own two
// negatives, the K rows of the memory bank) and its gradients with respect to q, q_sp, [c1; c2] and the negatives
// (include/mdr_inbatch_loss.h: mdr_inbatch_loss_forward / mdr_inbatch_loss_backward). No score, probability or mask matrix is formed.
//
// Forward.  loss_queue_lse_kernel folds the queue columns of a chunk of 128 column tiles into one (max, sum) pair per row and
//   chunk; loss_forward_kernel is the sweep of the rank step (same tile code, same wave order, same merges, hence the same
//   bits when K = 0) and merges the chunk pairs, in chunk order, after the two negatives.
// Backward. g_ij = (exp(s_ij - lse_i) - [j = t_i]) * g0 / B, 0 at the masked column; g0 is read from the device.
//   loss_grad_sweep_kernel<.., false> (row pass): a workgroup owns 32 query rows of one hop and one chunk of 128 column tiles;
//   loss_grad_sweep_kernel<.., true>  (column pass): a workgroup owns 32 rows of [c1; c2] and sweeps a chunk of one hop's queries.
//   A step takes 128 swept vectors: each wave recomputes the 16 x 32 score tile of its 16 vectors on MFMA (tile_mma), turns it
//   into g and stores it in LDS; after a barrier each wave owns 32-wide slices of d and contracts g (32 x 128, from LDS) with the
//   128 swept vectors (from global memory, their row pointers passed through LDS) on MFMA into its accumulators. The sums of a
//   chunk go to the workspace; loss_row_finish_kernel / loss_col_finish_kernel add the chunks in chunk order, the two negatives
//   (row pass) and the two hops (column pass). Every output element has one owner and one summation order: no atomics, and
//   two runs give the same bits.
//
// Rounding points of mode O1 (apex O1 as remembered, not captured: apex cannot be installed offline; criterions.py says the
// same of the forward). torch.mm / torch.bmm are patched to cast their fp32 operands to fp16, CrossEntropyLoss runs in fp32:
//   1. every score is fp16(fp32 sum of fp16(x) * fp16(y)); lse and p = exp(s - lse) are fp32 over those values;
//   2. g is rounded to fp16 once: the backward of the .float() amp puts in front of the loss;
//   3. the backward of one mm / bmm call contracts fp16 g with the fp16-rounded other operand in fp32 and rounds the sum to fp16
//      once, then widens it (the backward of the cast of the fp32 leaf). The calls are: hop-1 mm, hop-2 mm (each gives a term
//      of dq or dq_sp and a term of d[c1; c2]), the two queue mms (a term of dq / dq_sp only), the two bmms (a term of
//      dq / dq_sp and a term of dneg each);
//   4. the terms of one leaf are added in fp32: ctx term + queue term + negatives term for dq, hop 1 + hop 2 for dctx and dneg.
#include "mdr_inbatch_tile.h"

namespace mdr {
namespace {

constexpr int kGrChunkTiles = 128;            // 16-vector sweep tiles per workgroup: 16 steps of 8 tiles
constexpr int kGrStep = kIbWaves * 16;        // swept vectors per step
constexpr int kGrUnits = kIbMaxD / 32 / kIbWaves;  // 32-wide slices of d per wave
constexpr int kGrMaxChunks = 65535;
constexpr int kFinThreads = 256;

template <int MODE>
struct GrG {  // the g tile in LDS, [32 owners][128 swept + pad]
    using T = float;
    static constexpr int STRIDE = kGrStep + 4;
};
template <>
struct GrG<MDR_INBATCH_O1> {
    using T = _Float16;
    static constexpr int STRIDE = kGrStep + 8;
};

template <int MODE>
__device__ __forceinline__ float gr_round(float x) {
    return MODE == MDR_INBATCH_O1 ? (float)(_Float16)x : x;
}

// stage 32 rows of X (rows past n repeat row n - 1: computed, never written), mode O1 rounded to fp16
template <int MODE>
__device__ __forceinline__ void stage_rows(const float* __restrict__ X, int row0, int n, int d, typename IbElem<MODE>::T* xt, int stride, int tid) {
    using T = typename IbElem<MODE>::T;
    const int d4 = d >> 2;
    for (int idx = tid; idx < kIbQT * d4; idx += kIbThreads) {
        const int r = idx / d4, c4 = idx - r * d4;
        const int xr = min(row0 + r, n - 1);
        const float4 v = *(const float4*)(X + (size_t)xr * d + 4 * c4);
        T* dst = xt + r * stride + 4 * c4;
        dst[0] = (T)v.x;
        dst[1] = (T)v.y;
        dst[2] = (T)v.z;
        dst[3] = (T)v.w;
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int MODE>
__global__ void __launch_bounds__(kIbThreads)
loss_queue_lse_kernel(const float* __restrict__ q, const float* __restrict__ qsp, const float* __restrict__ queue, long long K, int B, int d,
                      float* __restrict__ pm, float* __restrict__ ps) {
    using T = typename IbElem<MODE>::T;
    extern __shared__ __attribute__((aligned(16))) char ib_lds[];
    T* qt = (T*)ib_lds;
    __shared__ float p_m[kIbWaves][kIbQT], p_s[kIbWaves][kIbQT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int hop = blockIdx.y, q0 = blockIdx.x * kIbQT, chunk = blockIdx.z;
    const int stride = d + IbElem<MODE>::PAD;
    stage_rows<MODE>(hop ? qsp : q, q0, B, d, qt, stride, tid);
    __syncthreads();

    const long long nqt = (K + 15) >> 4;
    const long long tile0 = (long long)chunk * kGrChunkTiles;
    const long long tile1 = tile0 + kGrChunkTiles < nqt ? tile0 + kGrChunkTiles : nqt;
    float m[2] = {-INFINITY, -INFINITY}, s[2] = {0.f, 0.f};
    for (long long tile = tile0 + wave; tile < tile1; tile += kIbWaves) {
        const long long arow = 16 * tile + c < K ? 16 * tile + c : K - 1;
        ib_f32x4 acc[2];
        tile_mma<MODE>(queue + (size_t)arow * d, qt, stride, d, lane, acc[0], acc[1]);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (16 * tile + 4 * g + r < K) lse_fold(m[u], s[u], ib_score<MODE>(acc[u][r]));
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float m2 = __shfl_xor(m[u], off), s2 = __shfl_xor(s[u], off);
            lse_merge(m[u], s[u], m2, s2);
        }
        if (g == 0) {
            p_m[wave][16 * u + c] = m[u];
            p_s[wave][16 * u + c] = s[u];
        }
    }
    __syncthreads();
    if (tid < kIbQT && q0 + tid < B) {
        float M = -INFINITY, S = 0.f;
        for (int w = 0; w < kIbWaves; ++w) lse_merge(M, S, p_m[w][tid], p_s[w][tid]);
        const size_t o = ((size_t)chunk * 2 + hop) * B + q0 + tid;
        pm[o] = M;
        ps[o] = S;
    }
}

// The rank step's kernel without the rank counts (csrc/mdr_inbatch.hip: same staging, same negatives, same target tiles, same
// sweep and merges), followed by the queue chunks' (max, sum) pairs.
template <int MODE>
__global__ void __launch_bounds__(kIbThreads)
loss_forward_kernel(const float* __restrict__ q, const float* __restrict__ qsp, const float* __restrict__ ctx, const float* __restrict__ neg,
                    int B, int d, const float* __restrict__ pm, const float* __restrict__ ps, int nqchunks, float* __restrict__ tscore1,
                    float* __restrict__ tscore2, float* __restrict__ lse1, float* __restrict__ lse2) {
    using T = typename IbElem<MODE>::T;
    extern __shared__ __attribute__((aligned(16))) char ib_lds[];
    T* qt = (T*)ib_lds;  // [kIbQT][d + PAD]
    __shared__ float p_m[kIbWaves][kIbQT], p_s[kIbWaves][kIbQT];
    __shared__ float p_ts[kIbQT], p_neg[kIbQT][2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int hop = blockIdx.y, q0 = blockIdx.x * kIbQT;
    const int stride = d + IbElem<MODE>::PAD;
    stage_rows<MODE>(hop ? qsp : q, q0, B, d, qt, stride, tid);
    __syncthreads();

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

    float ts[2];
    {
        const float* sec_base = ctx + (size_t)hop * B * d;
        ib_f32x4 a0, a1, b0, b1;
        const int row0 = min(q0 + c, B - 1), row1 = min(q0 + 16 + c, B - 1);
        tile_mma<MODE>(sec_base + (size_t)row0 * d, qt, stride, d, lane, a0, a1);
        tile_mma<MODE>(sec_base + (size_t)row1 * d, qt, stride, d, lane, b0, b1);
        const int src = 16 * (c >> 2) + c;
        ts[0] = ib_score<MODE>(__shfl(pick4(a0, c & 3), src));
        ts[1] = ib_score<MODE>(__shfl(pick4(b1, c & 3), src));
    }

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
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * t + 4 * g + r;
                const bool masked = hop == 0 && sec == 1 && row == qi;
                if (row < B && !masked) lse_fold(m[u], s[u], ib_score<MODE>(acc[u][r]));
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float m2 = __shfl_xor(m[u], off), s2 = __shfl_xor(s[u], off);
            lse_merge(m[u], s[u], m2, s2);
        }
        if (g == 0) {
            p_m[wave][16 * u + c] = m[u];
            p_s[wave][16 * u + c] = s[u];
            if (wave == 0) p_ts[16 * u + c] = ts[u];
        }
    }
    __syncthreads();

    if (tid < kIbQT && q0 + tid < B) {
        const int qi = q0 + tid;
        float M = -INFINITY, S = 0.f;
        for (int w = 0; w < kIbWaves; ++w) lse_merge(M, S, p_m[w][tid], p_s[w][tid]);
        for (int n = 0; n < 2; ++n) lse_fold(M, S, p_neg[tid][n]);
        for (int ch = 0; ch < nqchunks; ++ch) {
            const size_t o = ((size_t)ch * 2 + hop) * B + qi;
            lse_merge(M, S, pm[o], ps[o]);
        }
        (hop ? tscore2 : tscore1)[qi] = p_ts[tid];
        (hop ? lse2 : lse1)[qi] = M + logf(S);
    }
}

// --------------------------------------------------------------------------------------------------------------- backward
// COLPASS false: owners = the hop's query rows (X = q or q_sp, n_owner = B); chunks [0, nctx_chunks) sweep the 2 * ceil(B / 16)
//                tiles of [c1; c2] (each section tiled from its own row 0), chunks from nctx_chunks on sweep the queue tiles.
// COLPASS true:  owners = the rows of [c1; c2] (n_owner = 2B); the chunks sweep the ceil(B / 16) tiles of the hop's query rows.
// part: [chunk][hop][n_owner][d] fp32.
template <int MODE, bool COLPASS>
__global__ void __launch_bounds__(kIbThreads)
loss_grad_sweep_kernel(const float* __restrict__ q, const float* __restrict__ qsp, const float* __restrict__ ctx, const float* __restrict__ queue,
                       long long K, int B, int d, const float* __restrict__ lse1, const float* __restrict__ lse2, const float* __restrict__ g0,
                       int nctx_chunks, float* __restrict__ part) {
    using T = typename IbElem<MODE>::T;
    using GT = typename GrG<MODE>::T;
    constexpr int GS = GrG<MODE>::STRIDE;
    extern __shared__ __attribute__((aligned(16))) char ib_lds[];
    T* xt = (T*)ib_lds;  // [kIbQT][d + PAD]: the owners
    __shared__ __attribute__((aligned(16))) GT gt[kIbQT * GS];
    __shared__ __attribute__((aligned(16))) const float* rowptr[kGrStep];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int hop = blockIdx.y, o0 = blockIdx.x * kIbQT, chunk = blockIdx.z;
    const int stride = d + IbElem<MODE>::PAD;
    const int n_owner = COLPASS ? 2 * B : B;
    const float* Q = hop ? qsp : q;
    const float* lse = hop ? lse2 : lse1;
    stage_rows<MODE>(COLPASS ? ctx : Q, o0, n_owner, d, xt, stride, tid);

    const int nt = (B + 15) >> 4;
    const bool in_queue = !COLPASS && chunk >= nctx_chunks;
    const long long ntiles = COLPASS ? nt : in_queue ? (K + 15) >> 4 : 2 * nt;
    const long long tile0 = (long long)(in_queue ? chunk - nctx_chunks : chunk) * kGrChunkTiles;
    const long long tile1 = tile0 + kGrChunkTiles < ntiles ? tile0 + kGrChunkTiles : ntiles;
    const float scale = *g0 / (float)B;
    float lse_o[2] = {0.f, 0.f};
    if (!COLPASS) {
        lse_o[0] = lse[min(o0 + c, B - 1)];
        lse_o[1] = lse[min(o0 + 16 + c, B - 1)];
    }

    ib_f32x4 out[kGrUnits][2][2];
#pragma unroll
    for (int ui = 0; ui < kGrUnits; ++ui)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) out[ui][u][e2] = ib_f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();

    for (long long tbase = tile0; tbase < tile1; tbase += kIbWaves) {
        // ---- phase 1: this wave's 16 swept vectors x the 32 owners -> g in LDS ----
        {
            const bool live = tbase + wave < tile1;
            const long long tile = live ? tbase + wave : tile1 - 1;
            // the swept vector of tile row e: its pointer, whether it exists, its column (row pass) or query (column pass) number
            long long first;        // index of tile row 0 inside its section
            long long nsec;         // rows of the section
            const float* base;      // the section's row 0
            int jbase;              // column number of the section's row 0 (row pass)
            if (COLPASS) {
                first = 16 * tile, nsec = B, base = Q, jbase = 0;
            } else if (in_queue) {
                first = 16 * tile, nsec = K, base = queue, jbase = 2 * B + 2;
            } else {
                const int sec = tile >= nt ? 1 : 0;
                first = 16 * (tile - (long long)sec * nt), nsec = B, base = ctx + (size_t)sec * B * d, jbase = sec * B;
            }
            const long long arow = first + c < nsec ? first + c : nsec - 1;
            const float* ap = base + (size_t)arow * d;
            if (g == 0) rowptr[16 * wave + c] = ap;
            ib_f32x4 acc[2];
            tile_mma<MODE>(ap, xt, stride, d, lane, acc[0], acc[1]);
            float lse_s[4] = {0.f, 0.f, 0.f, 0.f};
            if (COLPASS) {
#pragma unroll
                for (int r = 0; r < 4; ++r) lse_s[r] = lse[first + 4 * g + r < B ? first + 4 * g + r : B - 1];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int owner = o0 + 16 * u + c;
                float gv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long row = first + 4 * g + r;
                    const long long qi = COLPASS ? row : owner;            // the query of this score
                    const long long j = COLPASS ? owner : jbase + row;     // its column
                    const bool in_batch = COLPASS || !in_queue;
                    const bool masked = in_batch && hop == 0 && j == B + qi;
                    const bool target = in_batch && j == (long long)hop * B + qi;
                    const float sc = ib_score<MODE>(acc[u][r]);
                    const float p = expf(sc - (COLPASS ? lse_s[r] : lse_o[u]));
                    const float v = (p - (target ? 1.f : 0.f)) * scale;
                    gv[r] = (live && row < nsec && !masked) ? gr_round<MODE>(v) : 0.f;
                }
                GT* dst = gt + (16 * u + c) * GS + 16 * wave + 4 * g;
                dst[0] = (GT)gv[0];
                dst[1] = (GT)gv[1];
                dst[2] = (GT)gv[2];
                dst[3] = (GT)gv[3];
            }
        }
        __syncthreads();

        // ---- phase 2: out[owner][this wave's slices of d] += g[owner][128] . swept[128][slice] ----
        if (32 * wave < d) {
            if (MODE == MDR_INBATCH_F32) {
                // 16x16x4: MFMA e of a 16-wide step sums swept vector k0 + 4 * slot + e over the slots, the permutation A and B share
#pragma unroll 2
                for (int k0 = 0; k0 < kGrStep; k0 += 16) {
                    const float4 ga0 = *(const float4*)((const float*)gt + c * GS + k0 + 4 * g);
                    const float4 ga1 = *(const float4*)((const float*)gt + (16 + c) * GS + k0 + 4 * g);
                    const float* rp[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) rp[e] = rowptr[k0 + 4 * g + e];
                    const float a0[4] = {ga0.x, ga0.y, ga0.z, ga0.w}, a1[4] = {ga1.x, ga1.y, ga1.z, ga1.w};
#pragma unroll
                    for (int ui = 0; ui < kGrUnits; ++ui) {
                        const int off = 32 * (wave + kIbWaves * ui);
                        if (off < d) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float2 b = *(const float2*)(rp[e] + off + 2 * c);  // output column c of n-subtile e2 is d index off + 2c + e2
                                out[ui][0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b.x, out[ui][0][0], 0, 0, 0);
                                out[ui][0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b.y, out[ui][0][1], 0, 0, 0);
                                out[ui][1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b.x, out[ui][1][0], 0, 0, 0);
                                out[ui][1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b.y, out[ui][1][1], 0, 0, 0);
                            }
                        }
                    }
                }
            } else {
                for (int k0 = 0; k0 < kGrStep; k0 += 32) {
                    const ib_half8 ga0 = *(const ib_half8*)((const _Float16*)gt + c * GS + k0 + 8 * g);
                    const ib_half8 ga1 = *(const ib_half8*)((const _Float16*)gt + (16 + c) * GS + k0 + 8 * g);
                    const float* rp[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) rp[e] = rowptr[k0 + 8 * g + e];
#pragma unroll
                    for (int ui = 0; ui < kGrUnits; ++ui) {
                        const int off = 32 * (wave + kIbWaves * ui);
                        if (off < d) {
                            ib_half8 b0, b1;
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const float2 b = *(const float2*)(rp[e] + off + 2 * c);
                                b0[e] = (_Float16)b.x;
                                b1[e] = (_Float16)b.y;
                            }
                            out[ui][0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga0, b0, out[ui][0][0], 0, 0, 0);
                            out[ui][0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga0, b1, out[ui][0][1], 0, 0, 0);
                            out[ui][1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga1, b0, out[ui][1][0], 0, 0, 0);
                            out[ui][1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga1, b1, out[ui][1][1], 0, 0, 0);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- this chunk's sums: C[row 4g + r = owner][col c = d index off + 2c + e2] ----
    float* dst = part + ((size_t)chunk * 2 + hop) * n_owner * d;
#pragma unroll
    for (int ui = 0; ui < kGrUnits; ++ui) {
        const int off = 32 * (wave + kIbWaves * ui);
        if (off < d) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int owner = o0 + 16 * u + 4 * g + r;
                    if (owner < n_owner) *(float2*)(dst + (size_t)owner * d + off + 2 * c) = float2{out[ui][u][0][r], out[ui][u][1][r]};
                }
            }
        }
    }
}

// One workgroup per batch row i: the four scores of the row's two negatives, their g, dneg[i], and dq[i] / dqsp[i] = the
// context chunks + the queue chunks + the negatives' term.
template <int MODE>
__global__ void __launch_bounds__(kFinThreads)
loss_row_finish_kernel(const float* __restrict__ q, const float* __restrict__ qsp, const float* __restrict__ neg, int B, int d,
                       const float* __restrict__ lse1, const float* __restrict__ lse2, const float* __restrict__ g0, const float* __restrict__ part,
                       int nctx_chunks, int nq_chunks, float* __restrict__ dq, float* __restrict__ dqsp, float* __restrict__ dneg) {
    __shared__ float red[kFinThreads / 64][4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* x[2] = {q + (size_t)i * d, qsp + (size_t)i * d};
    const float* n[2] = {neg + (size_t)i * 2 * d, neg + ((size_t)i * 2 + 1) * d};
    float dot[4] = {0.f, 0.f, 0.f, 0.f};  // [hop][negative]
    for (int k = tid; k < d; k += kFinThreads) {
        const float x0 = gr_round<MODE>(x[0][k]), x1 = gr_round<MODE>(x[1][k]);
        const float n0 = gr_round<MODE>(n[0][k]), n1 = gr_round<MODE>(n[1][k]);
        dot[0] = fmaf(x0, n0, dot[0]);
        dot[1] = fmaf(x0, n1, dot[1]);
        dot[2] = fmaf(x1, n0, dot[2]);
        dot[3] = fmaf(x1, n1, dot[3]);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) dot[v] += __shfl_xor(dot[v], off);
        if ((tid & 63) == 0) red[tid >> 6][v] = dot[v];
    }
    __syncthreads();
    const float scale = *g0 / (float)B;
    const float l[2] = {lse1[i], lse2[i]};
    float gn[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        float s = red[0][v];
        for (int w = 1; w < kFinThreads / 64; ++w) s += red[w][v];
        gn[v] = gr_round<MODE>(expf(ib_score<MODE>(s) - l[v >> 1]) * scale);  // a negative is never a target and never masked
    }
    const size_t slab = (size_t)2 * B * d;
    for (int k = tid; k < d; k += kFinThreads) {
        const float x0 = gr_round<MODE>(x[0][k]), x1 = gr_round<MODE>(x[1][k]);
        const float n0 = gr_round<MODE>(n[0][k]), n1 = gr_round<MODE>(n[1][k]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* p = part + ((size_t)h * B + i) * d + k;
            float a = 0.f, b = 0.f;
            for (int z = 0; z < nctx_chunks; ++z) a += p[z * slab];
            for (int z = 0; z < nq_chunks; ++z) b += p[(nctx_chunks + z) * slab];
            const float t = gn[2 * h] * n0 + gn[2 * h + 1] * n1;
            float r = gr_round<MODE>(a);
            if (nq_chunks) r += gr_round<MODE>(b);
            r += gr_round<MODE>(t);
            (h ? dqsp : dq)[(size_t)i * d + k] = r;
        }
        dneg[((size_t)i * 2) * d + k] = gr_round<MODE>(gn[0] * x0) + gr_round<MODE>(gn[2] * x1);
        dneg[((size_t)i * 2 + 1) * d + k] = gr_round<MODE>(gn[1] * x0) + gr_round<MODE>(gn[3] * x1);
    }
}

// dctx[j] = hop-1 chunks + hop-2 chunks, each hop's sum rounded on its own in mode O1
template <int MODE>
__global__ void __launch_bounds__(kFinThreads)
loss_col_finish_kernel(const float* __restrict__ part, int B, int d, int nchunks, float* __restrict__ dctx) {
    const size_t n = (size_t)2 * B * d;
    const size_t e = (size_t)blockIdx.x * kFinThreads + threadIdx.x;
    if (e >= n) return;
    float a[2] = {0.f, 0.f};
    for (int z = 0; z < nchunks; ++z) {
        a[0] += part[((size_t)z * 2) * n + e];
        a[1] += part[((size_t)z * 2 + 1) * n + e];
    }
    dctx[e] = gr_round<MODE>(a[0]) + gr_round<MODE>(a[1]);
}

// ------------------------------------------------------------------------------------------------------------------- host
struct GrPlan {
    int nt, nctx_chunks, nq_chunks, ncol_chunks;
    size_t fwd_bytes, bwd_bytes;
};

bool gr_shape_ok(int B, int d, long long K, int mode) {
    return B >= 1 && B <= (1 << 24) && d >= 32 && d <= kIbMaxD && d % 32 == 0 && K >= 0 && K <= ((long long)1 << 26) &&
           (mode == MDR_INBATCH_F32 || mode == MDR_INBATCH_O1);
}

GrPlan gr_plan(int B, int d, long long K) {
    GrPlan p;
    p.nt = (B + 15) >> 4;
    p.nctx_chunks = (2 * p.nt + kGrChunkTiles - 1) / kGrChunkTiles;
    p.nq_chunks = (int)((((K + 15) >> 4) + kGrChunkTiles - 1) / kGrChunkTiles);
    p.ncol_chunks = (p.nt + kGrChunkTiles - 1) / kGrChunkTiles;
    p.fwd_bytes = (size_t)p.nq_chunks * 2 * B * 2 * sizeof(float);
    const size_t row = (size_t)(p.nctx_chunks + p.nq_chunks) * 2 * B * d * sizeof(float);
    const size_t col = (size_t)p.ncol_chunks * 2 * 2 * B * d * sizeof(float);
    p.bwd_bytes = row > col ? row : col;
    return p;
}

template <int MODE>
int launch_loss_forward(const float* q, const float* qsp, const float* ctx, const float* neg, const float* queue, long long K, int B, int d,
                        float* ts1, float* ts2, float* lse1, float* lse2, float* ws, hipStream_t stream) {
    using T = typename IbElem<MODE>::T;
    const GrPlan p = gr_plan(B, d, K);
    const int lds = kIbQT * (d + IbElem<MODE>::PAD) * (int)sizeof(T);
    const int lds_max = kIbQT * (kIbMaxD + IbElem<MODE>::PAD) * (int)sizeof(T);
    const unsigned qtiles = (unsigned)((B + kIbQT - 1) / kIbQT);
    float* pm = ws;
    float* ps = ws ? ws + (size_t)p.nq_chunks * 2 * B : nullptr;
    int rc;
    if (p.nq_chunks) {
        if ((rc = ensure_dynamic_lds((const void*)loss_queue_lse_kernel<MODE>, lds_max)) != MDR_OK) return rc;
        hipLaunchKernelGGL(loss_queue_lse_kernel<MODE>, dim3(qtiles, 2, (unsigned)p.nq_chunks), dim3(kIbThreads), lds, stream, q, qsp, queue, K, B, d, pm, ps);
        MDR_HIP_TRY(hipGetLastError());
    }
    if ((rc = ensure_dynamic_lds((const void*)loss_forward_kernel<MODE>, lds_max)) != MDR_OK) return rc;
    hipLaunchKernelGGL(loss_forward_kernel<MODE>, dim3(qtiles, 2), dim3(kIbThreads), lds, stream, q, qsp, ctx, neg, B, d, (const float*)pm,
                       (const float*)ps, p.nq_chunks, ts1, ts2, lse1, lse2);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

template <int MODE>
int launch_loss_backward(const float* q, const float* qsp, const float* ctx, const float* neg, const float* queue, long long K, int B, int d,
                         const float* lse1, const float* lse2, const float* g0, float* dq, float* dqsp, float* dctx, float* dneg, float* ws,
                         hipStream_t stream) {
    using T = typename IbElem<MODE>::T;
    const GrPlan p = gr_plan(B, d, K);
    const int lds = kIbQT * (d + IbElem<MODE>::PAD) * (int)sizeof(T);
    const int lds_max = kIbQT * (kIbMaxD + IbElem<MODE>::PAD) * (int)sizeof(T);
    int rc;
    if ((rc = ensure_dynamic_lds((const void*)loss_grad_sweep_kernel<MODE, false>, lds_max)) != MDR_OK) return rc;
    if ((rc = ensure_dynamic_lds((const void*)loss_grad_sweep_kernel<MODE, true>, lds_max)) != MDR_OK) return rc;
    // the row pass and its finish, then the column pass and its finish: the two passes share the workspace, in stream order
    hipLaunchKernelGGL((loss_grad_sweep_kernel<MODE, false>), dim3((unsigned)((B + kIbQT - 1) / kIbQT), 2, (unsigned)(p.nctx_chunks + p.nq_chunks)),
                       dim3(kIbThreads), lds, stream, q, qsp, ctx, queue, K, B, d, lse1, lse2, g0, p.nctx_chunks, ws);
    MDR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loss_row_finish_kernel<MODE>, dim3((unsigned)B), dim3(kFinThreads), 0, stream, q, qsp, neg, B, d, lse1, lse2, g0, (const float*)ws,
                       p.nctx_chunks, p.nq_chunks, dq, dqsp, dneg);
    MDR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((loss_grad_sweep_kernel<MODE, true>), dim3((unsigned)((2 * B + kIbQT - 1) / kIbQT), 2, (unsigned)p.ncol_chunks), dim3(kIbThreads), lds,
                       stream, q, qsp, ctx, queue, K, B, d, lse1, lse2, g0, 0, ws);
    MDR_HIP_TRY(hipGetLastError());
    const size_t n = (size_t)2 * B * d;
    hipLaunchKernelGGL(loss_col_finish_kernel<MODE>, dim3((unsigned)((n + kFinThreads - 1) / kFinThreads)), dim3(kFinThreads), 0, stream, (const float*)ws, B,
                       d, p.ncol_chunks, dctx);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int loss_check(const char* fn, const void* q, const void* qsp, const void* ctx, const void* neg, const void* queue, long long K, int B, int d, int mode,
               const void* ws, size_t bytes, size_t need) {
    MDR_REQUIRE(B >= 1, "%s: B = %d, need B >= 1", fn, B);
    MDR_REQUIRE(K >= 0, "%s: K = %lld, need K >= 0", fn, K);
    MDR_REQUIRE(mode == MDR_INBATCH_F32 || mode == MDR_INBATCH_O1, "%s: unknown mode %d", fn, mode);
    MDR_REQUIRE(gr_shape_ok(B, d, K, mode), "%s: B = %d, d = %d, K = %lld unsupported (d a multiple of 32 in [32, %d], B <= 2^24, K <= 2^26)", fn, B, d, K,
                kIbMaxD);
    MDR_REQUIRE(gr_plan(B, d, K).nctx_chunks + gr_plan(B, d, K).nq_chunks <= kGrMaxChunks, "%s: B = %d, K = %lld: too many column chunks", fn, B, K);
    MDR_REQUIRE(q && qsp && ctx && neg, "%s: q, qsp, ctx and neg must not be NULL", fn);
    MDR_REQUIRE(K == 0 || queue, "%s: queue must not be NULL when K = %lld", fn, K);
    MDR_REQUIRE(aligned16({q, qsp, ctx, neg, queue}), "%s: q, qsp, ctx, neg and queue must be 16-byte aligned", fn);
    MDR_REQUIRE(need == 0 || (ws && bytes >= need), "%s: workspace of %zu bytes, need %zu", fn, ws ? bytes : (size_t)0, need);
    MDR_REQUIRE(aligned16({ws}), "%s: the workspace must be 16-byte aligned", fn);
    return MDR_OK;
}

}  // namespace
}  // namespace mdr

extern "C" {

size_t mdr_inbatch_loss_workspace_bytes(int B, int d, int64_t K, int mode) {
    using namespace mdr;
    if (!gr_shape_ok(B, d, K, mode)) return 0;
    const GrPlan p = gr_plan(B, d, K);
    return align_up(p.fwd_bytes > p.bwd_bytes ? p.fwd_bytes : p.bwd_bytes, 256);
}

int mdr_inbatch_loss_forward(const float* q_dev, const float* qsp_dev, const float* ctx_dev, const float* neg_dev, const float* queue_dev, int64_t K,
                             int B, int d, int mode, float* tscore1_dev, float* tscore2_dev, float* lse1_dev, float* lse2_dev, void* workspace_dev,
                             size_t workspace_bytes, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_inbatch_loss_forward";
    const size_t need = gr_shape_ok(B, d, K, mode) ? gr_plan(B, d, K).fwd_bytes : 0;
    int rc = loss_check(fn, q_dev, qsp_dev, ctx_dev, neg_dev, queue_dev, K, B, d, mode, workspace_dev, workspace_bytes, need);
    if (rc != MDR_OK) return rc;
    MDR_REQUIRE(tscore1_dev && tscore2_dev && lse1_dev && lse2_dev, "%s: tscore1, tscore2, lse1 and lse2 must not be NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace_dev;
    if (mode == MDR_INBATCH_O1)
        return launch_loss_forward<MDR_INBATCH_O1>(q_dev, qsp_dev, ctx_dev, neg_dev, queue_dev, K, B, d, tscore1_dev, tscore2_dev, lse1_dev, lse2_dev, ws, st);
    return launch_loss_forward<MDR_INBATCH_F32>(q_dev, qsp_dev, ctx_dev, neg_dev, queue_dev, K, B, d, tscore1_dev, tscore2_dev, lse1_dev, lse2_dev, ws, st);
}

int mdr_inbatch_loss_backward(const float* q_dev, const float* qsp_dev, const float* ctx_dev, const float* neg_dev, const float* queue_dev, int64_t K,
                              int B, int d, int mode, const float* lse1_dev, const float* lse2_dev, const float* g0_dev, float* dq_dev, float* dqsp_dev,
                              float* dctx_dev, float* dneg_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_inbatch_loss_backward";
    const size_t need = gr_shape_ok(B, d, K, mode) ? gr_plan(B, d, K).bwd_bytes : 0;
    int rc = loss_check(fn, q_dev, qsp_dev, ctx_dev, neg_dev, queue_dev, K, B, d, mode, workspace_dev, workspace_bytes, need);
    if (rc != MDR_OK) return rc;
    MDR_REQUIRE(lse1_dev && lse2_dev && g0_dev, "%s: lse1, lse2 and g0 must not be NULL", fn);
    MDR_REQUIRE(dq_dev && dqsp_dev && dctx_dev && dneg_dev, "%s: dq, dqsp, dctx and dneg must not be NULL", fn);
    MDR_REQUIRE(aligned16({dq_dev, dqsp_dev, dctx_dev, dneg_dev}), "%s: dq, dqsp, dctx and dneg must be 16-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace_dev;
    if (mode == MDR_INBATCH_O1)
        return launch_loss_backward<MDR_INBATCH_O1>(q_dev, qsp_dev, ctx_dev, neg_dev, queue_dev, K, B, d, lse1_dev, lse2_dev, g0_dev, dq_dev, dqsp_dev, dctx_dev,
                                                    dneg_dev, ws, st);
    return launch_loss_backward<MDR_INBATCH_F32>(q_dev, qsp_dev, ctx_dev, neg_dev, queue_dev, K, B, d, lse1_dev, lse2_dev, g0_dev, dq_dev, dqsp_dev, dctx_dev,
                                                 dneg_dev, ws, st);
}

}  // extern "C"
