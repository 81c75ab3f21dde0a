// csrc/mdr_attention_grad.hip -- the backward of self-attention on the packed, ragged rows of the trunk (include/mdr_attention_grad.h:
// mdr_attention_backward). Per (sequence, head), s = Q K^T / 8, p = softmax(s) over the sequence's own keys, dO = the head's slice of dctx:
//     dV = p^T dO     dP = dO V^T     delta_i = sum_j p_ij dP_ij     dS = p o (dP - delta)     dQ = dS K / 8     dK = dS^T Q / 8
// No score, probability or dS matrix goes to memory: S and dP are recomputed on MFMA wherever they are needed. The only scratch is one
// (lse, delta) fp32 pair per (token, head).
//
// attn_grad_kernel<false> (row pass): a workgroup of four waves owns 64 queries of one (sequence, head), 16 per wave, their Q and dO rows in
//   registers as MFMA B operands, and sweeps the sequence's keys in chunks of 64 (K and V rows staged in LDS, 128-byte rows, 16-byte slots
//   XOR-swizzled by row & 7, rows past the sequence zero). Sweep 0 folds the chunks into a running (max, sum, sum of e dP) per query and
//   writes lse = max + log(sum) and delta = sum of e dP / sum to the workspace. Sweep 1 forms p = exp(s - lse), dS = p (dP - delta) and
//   accumulates dQ^T = K^T dS^T: the dS operand is the lane's own S^T registers, the K^T operand two transposing reads of the row-major
//   image (ds_read_b64_tr_b16, the addressing of the forward's streaming kernel).
// attn_grad_kernel<true> (column pass): the same code with the roles exchanged. A workgroup owns 64 keys (K and V rows in registers) and
//   sweeps the sequence's queries in chunks of 64 (Q and dO rows and their (lse, delta) pairs staged in LDS); it accumulates dV^T = dO^T P
//   and dK^T = Q^T dS.
// attn_grad_cls_kernel (mode 3): the forward computed only the first query of each sequence. One workgroup per (sequence, head), no MFMA:
//   scores and dP of the one query over the keys, softmax, delta, then dK and dV rows (outer products), zeros in the other dQ rows, and
//   dQ of row cu[b] as four strided partial sums added in a fixed order.
// Every output element has one owner and one summation order: no atomics, and two runs give the same bits. S and dP are computed three
// times (sweep 0, sweep 1, column pass) where a backward that adds dQ with atomics computes them once: the price of that.
//
// Rounding points (tests/attention_grad_ref.py derives its bound from this list):
//   1. Q, K, V and dO are fp16: exact operands. A product of two fp16 is exact in fp32.
//   2. s = fp32 sum of 64 products (MFMA; mode 3: an fma chain) times 1/8 (exact). dP likewise, without the factor.
//   3. lse and delta, fp32. Mode 0: e = v_exp_f32(fma(s, log2 e, -m log2 e)) against the running maximum m of the chunks so far; a later
//      chunk multiplies sum and sum of e dP by alpha = exp2((m_old - m_new) log2 e); lse = m + logf(sum), delta = (sum of e dP) / sum.
//      Mode 3: e = exp2((s - max) log2 e), p = e * (1 / sum), delta = (sum of e dP) * (1 / sum).
//   4. p = v_exp_f32((s - lse) log2 e) in fp32 (mode 0, in both passes, from the stored lse); dS = p * (dP - delta) in fp32.
//   5. p is rounded to fp16 ONLY as the MFMA operand of dV; dS is rounded to fp16 ONLY as the operand of dQ and dK.
//   6. dQ, dK, dV accumulate in fp32 (MFMA; mode 3: dQ as fma chains, dK and dV single products); dQ and dK are multiplied by 1/8 (exact)
//      and every output is rounded to fp16 once.
//
// Dropout (include/mdr_dropout.h: mdr_attention_dropout_forward, mdr_attention_dropout_backward; the mask function is csrc/mdr_dropout.h's).
// attn_drop_fwd_kernel is the training forward, ctx = (p o m) V: the row pass with other operands. attn_grad_kernel<*, true> and
// attn_grad_cls_kernel<true> are its backward: dP is multiplied by m right after it is formed, in all three places S and dP are recomputed,
// and the dV operand is p * m; the mask is drawn again from (seed, site), never stored. The <*, false> instantiations are the kernels above,
// bit for bit. Rounding points of the dropout kernels (tests/dropout_ref.py derives its bound from 1 - 8):
//   1 - 6 as above: the forward computes s and lse (3. without the sum of e dP) and p (4.) with the instructions of the backward's sweeps.
//   7. m is 0 or fp32(256 / (256 - T)). dP * m and Pd = p * m are fp32 products (a multiplication, never a select: 0 * Inf = NaN). Pd is
//      rounded to fp16 ONLY as the MFMA operand of ctx (forward) and of dV (backward); mode 3 rounds fp16(p * m) likewise.
//   8. ctx accumulates in fp32 (MFMA; mode 3: fma chains, four strided partial sums added in wave order) and is rounded to fp16 once.
#include "mdr_dropout.h"
#include "mdr_grad_common.h"
#include "../../include/mdr_attention_grad.h"
#include "../../include/mdr_dropout.h"

namespace mdr {
namespace {

typedef _Float16 ag_half8 __attribute__((ext_vector_type(8)));
typedef _Float16 ag_half4 __attribute__((ext_vector_type(4)));
typedef float ag_f32x4 __attribute__((ext_vector_type(4)));
typedef __fp16 ag_fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

constexpr int kAgOwn = 64;                  // owners (queries in the row pass, keys in the column pass) per workgroup
constexpr int kAgWaves = kAgOwn / 16;       // 16 owners per wave
constexpr int kAgThreads = 64 * kAgWaves;
constexpr int kAgChunk = 64;                // swept rows per step: two pair-tiles of 32
constexpr int kAgTiles = kAgChunk / 16;
constexpr int kAgImage = kAgChunk * 128;    // bytes of one staged image
constexpr int kAgClsThreads = 256;
constexpr float kLog2e = 1.4426950408889634f;

// one image: rows row0 .. row0 + 63 of a sequence (64 halfs at `src` + row * stride), rows past the sequence zero
__device__ __forceinline__ void ag_stage(const _Float16* __restrict__ src, size_t stride, int row0, int len, char* img, int tid) {
    const ag_half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    ag_half8 v[kAgChunk * 8 / kAgThreads];
#pragma unroll
    for (int u = 0; u < kAgChunk * 8 / kAgThreads; ++u) {
        const int p = tid + u * kAgThreads, row = p >> 3, s = p & 7;
        v[u] = zero8;
        if (row0 + row < len) v[u] = *(const ag_half8*)(src + (size_t)(row0 + row) * stride + s * 8);
    }
#pragma unroll
    for (int u = 0; u < kAgChunk * 8 / kAgThreads; ++u) {
        const int p = tid + u * kAgThreads, row = p >> 3, s = p & 7;
        *(ag_half8*)(img + row * 128 + ((s ^ (row & 7)) << 4)) = v[u];
    }
}

// a1[t][r] = X1 . I1, a2[t][r] = X2 . I2 for swept row 16 t + 4 g + r of the chunk and owner lr (a1 times 1/8)
__device__ __forceinline__ void ag_tiles(const char* img1, const char* img2, const ag_half8 (&x1)[2], const ag_half8 (&x2)[2], int lane,
                                         ag_f32x4 (&a1)[kAgTiles], ag_f32x4 (&a2)[kAgTiles]) {
    const int g = lane >> 4, lr = lane & 15;
    const int rd = lr * 128, sw0 = (g ^ (lr & 7)) << 4, sw1 = ((4 + g) ^ (lr & 7)) << 4;
#pragma unroll
    for (int t = 0; t < kAgTiles; ++t) {
        const ag_half8 i10 = *(const ag_half8*)(img1 + t * 2048 + rd + sw0), i11 = *(const ag_half8*)(img1 + t * 2048 + rd + sw1);
        const ag_half8 i20 = *(const ag_half8*)(img2 + t * 2048 + rd + sw0), i21 = *(const ag_half8*)(img2 + t * 2048 + rd + sw1);
        ag_f32x4 s = {0.f, 0.f, 0.f, 0.f}, d = {0.f, 0.f, 0.f, 0.f};
        s = __builtin_amdgcn_mfma_f32_16x16x32_f16(i10, x1[0], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_f16(i11, x1[1], s, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(i20, x2[0], d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(i21, x2[1], d, 0, 0, 0);
        a1[t] = s * 0.125f;
        a2[t] = d;
    }
    // the callers read a2 behind a branch, where hipcc's hazard recogniser does not look for the distance a VALU read of an MFMA result needs
    asm volatile("s_nop 7\n\ts_nop 7" : "+v"(a2[0]), "+v"(a2[1]), "+v"(a2[2]), "+v"(a2[3]));
}

// acc[dt] (rows d = 16 dt + 4 g + r, column owner lr) += I^T . W over the 64 swept rows of the chunk: w[t][r] is the weight of swept row
// 16 t + 4 g + r. k-slot (g, j) of both operands <-> swept row 32 pt + (j < 4 ? 4 g + j : 16 + 4 g + j - 4): the weight operand is the
// lane's own registers, the I^T operand two transposing reads of the row-major image (lane a of a 16-lane group addresses row a >> 2,
// columns 4 (a & 3) .. of a [4 rows][16 d] block and receives column a).
__device__ __forceinline__ void ag_accumulate(const char* img, const ag_f32x4 (&w)[kAgTiles], int lane, ag_f32x4 (&acc)[4]) {
    const int g = lane >> 4, lr = lane & 15;
    const int vrow = 4 * g + (lr >> 2);
    const int rd = vrow * 128 + (lr & 1) * 8, sw = vrow & 7, half = (lr & 3) >> 1;
#pragma unroll
    for (int pt = 0; pt < kAgTiles / 2; ++pt) {
        ag_half8 wf;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wf[j] = (_Float16)w[2 * pt][j];
            wf[4 + j] = (_Float16)w[2 * pt + 1][j];
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const char* ip = img + pt * 4096 + rd + (((dt * 2 + half) ^ sw) << 4);
            const ag_fp16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) ag_fp16x4*)ip);
            const ag_fp16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) ag_fp16x4*)(ip + 2048));
            const ag_half8 it = {(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3],
                                 (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2], (_Float16)hi[3]};
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(it, wf, acc[dt], 0, 0, 0);
        }
    }
}

// out[owner lr][16 dt + 4 g + r] = fp16(acc[dt][r] * scale)
__device__ __forceinline__ void ag_store(ag_f32x4 (&acc)[4], float scale, _Float16* row, int g) {
    asm volatile("s_nop 7\n\ts_nop 7" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));  // (see attention_stream_kernel's epilogue)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        ag_half4 w;
#pragma unroll
        for (int r = 0; r < 4; ++r) w[r] = (_Float16)(acc[dt][r] * scale);
        *(ag_half4*)(row + dt * 16 + 4 * g) = w;
    }
}

// mk[t][r] = the dropout factor of swept row c0 + 16 t + 4 g + r and `owner` (csrc/mdr_dropout.h): a lane's four consecutive swept rows of one
// tile lie in one 4 x 4 block, so each tile costs one generator call. Row pass: owner = query, swept = keys; column pass: the reverse.
template <bool COLPASS>
__device__ __forceinline__ void ag_mask(int owner, int c0, int g, uint32_t bh, const DropoutParams& dpar, ag_f32x4 (&mk)[kAgTiles]) {
#pragma unroll
    for (int t = 0; t < kAgTiles; ++t) {
        const int blk = (c0 >> 2) + 4 * t + g;
        const uint32_t w = COLPASS ? dropout_attn_word_queries(blk, owner, bh, dpar) : dropout_attn_word_keys(owner, blk, bh, dpar);
#pragma unroll
        for (int r = 0; r < 4; ++r) mk[t][r] = dropout_factor(w, r, dpar);
    }
}

// stats: [heads][stat_stride] (lse, delta) pairs, indexed by the token's row in the packed batch
// DROP: the backward of the training forward below. dp is multiplied by the mask factor right after ag_tiles, wherever S and dP are recomputed,
// and the dV operand is p * m; nothing else changes.
template <bool COLPASS, bool DROP>
__global__ void __launch_bounds__(kAgThreads)
attn_grad_kernel(const _Float16* __restrict__ qkv, const _Float16* __restrict__ dctx, const int* __restrict__ cu, int H, size_t stat_stride,
                 float2* __restrict__ stats, _Float16* __restrict__ dqkv, DropoutParams dpar) {
    __shared__ __attribute__((aligned(128))) char img1[kAgImage];  // row pass: K rows; column pass: Q rows
    __shared__ __attribute__((aligned(128))) char img2[kAgImage];  // row pass: V rows; column pass: dO rows
    __shared__ __attribute__((aligned(16))) float2 st_s[kAgChunk];  // column pass: (lse, delta) of the chunk's queries
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, lr = lane & 15;
    const int h = blockIdx.x, b = blockIdx.y, o0 = blockIdx.z * kAgOwn;
    const int start = cu[b], len = cu[b + 1] - start;
    if (o0 >= len) return;  // (a sequence of length 0 has no workgroup that stays)
    const size_t H3 = (size_t)3 * H;
    const _Float16* seq = qkv + (size_t)start * H3 + h * 64;    // the sequence's Q rows of this head; + H: K, + 2 H: V
    const _Float16* dos = dctx + (size_t)start * H + h * 64;    // its dO rows
    float2* seq_stats = stats + (size_t)h * stat_stride + start;

    const int owner = o0 + wave * 16 + lr;
    const bool ovalid = owner < len;
    const int orow = ovalid ? owner : len - 1;         // owners past the sequence repeat its last row: computed, never written
    const bool wave_valid = o0 + wave * 16 < len;      // waves past the sequence only help staging
    ag_half8 x1[2], x2[2];
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) {
        if (COLPASS) {
            x1[ds] = *(const ag_half8*)(seq + (size_t)orow * H3 + H + ds * 32 + g * 8);
            x2[ds] = *(const ag_half8*)(seq + (size_t)orow * H3 + 2 * H + ds * 32 + g * 8);
        } else {
            x1[ds] = *(const ag_half8*)(seq + (size_t)orow * H3 + ds * 32 + g * 8);
            x2[ds] = *(const ag_half8*)(dos + (size_t)orow * H + ds * 32 + g * 8);
        }
    }
    const _Float16* src1 = COLPASS ? seq : seq + H;
    const _Float16* src2 = COLPASS ? dos : seq + 2 * H;
    const size_t stride2 = COLPASS ? (size_t)H : H3;

    ag_f32x4 acc1[4], acc2[4];  // row pass: dQ^T; column pass: dK^T and dV^T
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc1[dt] = acc2[dt] = (ag_f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f, d_run = 0.f, lse = 0.f, delta = 0.f;

    for (int sweep = COLPASS ? 1 : 0; sweep < 2; ++sweep) {
        for (int c0 = 0; c0 < len; c0 += kAgChunk) {
            if (sweep == 0 || COLPASS || len > kAgChunk) {  // (a sequence of one chunk: sweep 1 finds it staged)
                __syncthreads();                            // every wave is done with the previous chunk
                ag_stage(src1, H3, c0, len, img1, tid);
                ag_stage(src2, stride2, c0, len, img2, tid);
                if (COLPASS && tid < kAgChunk) st_s[tid] = c0 + tid < len ? seq_stats[c0 + tid] : float2{0.f, 0.f};
                __syncthreads();
            }
            if (!wave_valid) continue;
            ag_f32x4 s[kAgTiles], dp[kAgTiles];
            ag_tiles(img1, img2, x1, x2, lane, s, dp);
            ag_f32x4 mk[kAgTiles];  // DROP: the factor of swept row 16 t + 4 g + r and this owner
            if (DROP) {
                ag_mask<COLPASS>(owner, c0, g, (uint32_t)b * gridDim.x + h, dpar, mk);
#pragma unroll
                for (int t = 0; t < kAgTiles; ++t) dp[t] *= mk[t];
            }
            if (sweep == 0) {
                float cmax = -INFINITY;
#pragma unroll
                for (int t = 0; t < kAgTiles; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (c0 + 16 * t + 4 * g + r >= len) s[t][r] = -INFINITY;  // (a zero row: its dP is 0)
                        cmax = fmaxf(cmax, s[t][r]);
                    }
                cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
                cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
                const float m_new = fmaxf(m_run, cmax);  // finite: every chunk holds at least one key of the sequence
                const float alpha = exp2f((m_run - m_new) * kLog2e);  // 0 on the first chunk
                const float mb = -m_new * kLog2e;
                float csum = 0.f, dsum = 0.f;
#pragma unroll
                for (int t = 0; t < kAgTiles; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = __builtin_amdgcn_exp2f(fmaf(s[t][r], kLog2e, mb));  // argument <= 0 (up to rounding): raw v_exp_f32; -inf -> 0
                        csum += e;
                        dsum = fmaf(e, dp[t][r], dsum);
                    }
                csum += __shfl_xor(csum, 16);
                csum += __shfl_xor(csum, 32);
                dsum += __shfl_xor(dsum, 16);
                dsum += __shfl_xor(dsum, 32);
                l_run = l_run * alpha + csum;
                d_run = d_run * alpha + dsum;
                m_run = m_new;
            } else {
                ag_f32x4 p[kAgTiles], dsv[kAgTiles];
#pragma unroll
                for (int t = 0; t < kAgTiles; ++t) {
                    float ls[4], dl[4];
                    if (COLPASS) {
                        const float4 a = *(const float4*)&st_s[16 * t + 4 * g], c = *(const float4*)&st_s[16 * t + 4 * g + 2];
                        ls[0] = a.x, dl[0] = a.y, ls[1] = a.z, dl[1] = a.w, ls[2] = c.x, dl[2] = c.y, ls[3] = c.z, dl[3] = c.w;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool live = c0 + 16 * t + 4 * g + r < len;
                        const float e = __builtin_amdgcn_exp2f((s[t][r] - (COLPASS ? ls[r] : lse)) * kLog2e);
                        p[t][r] = live ? (DROP ? e * mk[t][r] : e) : 0.f;
                        dsv[t][r] = live ? e * (dp[t][r] - (COLPASS ? dl[r] : delta)) : 0.f;
                    }
                }
                ag_accumulate(img1, dsv, lane, acc1);
                if (COLPASS) ag_accumulate(img2, p, lane, acc2);
            }
        }
        if (sweep == 0) {
            lse = m_run + logf(l_run);
            delta = d_run / l_run;
            if (ovalid && g == 0) seq_stats[owner] = float2{lse, delta};
        }
    }
    if (!ovalid) return;
    _Float16* out = dqkv + (size_t)(start + owner) * H3 + h * 64;
    if (COLPASS) {
        ag_store(acc1, 0.125f, out + H, g);
        ag_store(acc2, 1.f, out + 2 * H, g);
    } else {
        ag_store(acc1, 0.125f, out, g);
    }
}

// the dropout factor of the first query and key `key` (mode 3: the attention site at i = 0)
__device__ __forceinline__ float ag_cls_factor(int key, uint32_t bh, const DropoutParams& dpar) {
    return dropout_factor(philox4x32_10(0u, (uint32_t)key >> 2, bh, dpar.site, dpar.k0, dpar.k1).x, key & 3, dpar);
}

// Mode 3: dctx is [B, H], the gradient of each sequence's first query alone. DROP: dP is multiplied by the mask factor where it is formed and
// the dV operand is fp16(p * m).
template <bool DROP>
__global__ void __launch_bounds__(kAgClsThreads)
attn_grad_cls_kernel(const _Float16* __restrict__ qkv, const _Float16* __restrict__ dctx, const int* __restrict__ cu, int H, _Float16* __restrict__ dqkv,
                     DropoutParams dpar) {
    constexpr int W = kAgClsThreads / 64;
    __shared__ float q_s[64], do_s[64];
    __shared__ float s_s[512], dp_s[512];  // scores, then fp16(p) (DROP: fp16(p m)); dP (DROP: dP m), then fp16(dS)
    __shared__ float m_s[DROP ? 512 : 1];  // DROP: the keys' factors
    __shared__ float red[3][W];
    __shared__ float part[W][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y;
    const int start = cu[b], len = cu[b + 1] - start;
    if (len <= 0) return;
    const size_t H3 = (size_t)3 * H;
    const _Float16* seq = qkv + (size_t)start * H3 + h * 64;
    if (tid < 64) {
        q_s[tid] = (float)seq[tid];
        do_s[tid] = (float)dctx[(size_t)b * H + h * 64 + tid];
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int key = tid; key < len; key += kAgClsThreads) {
        const _Float16* kp = seq + (size_t)key * H3 + H;
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const ag_half8 kv = *(const ag_half8*)(kp + c * 8), vv = *(const ag_half8*)(kp + H + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                s = fmaf((float)kv[j], q_s[c * 8 + j], s);
                dp = fmaf((float)vv[j], do_s[c * 8 + j], dp);
            }
        }
        s *= 0.125f;
        if (DROP) {
            const float m = ag_cls_factor(key, (uint32_t)b * gridDim.x + h, dpar);
            m_s[key] = m;
            dp *= m;
        }
        s_s[key] = s;
        dp_s[key] = dp;
        mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) red[0][wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    float sum = 0.f, dsum = 0.f;
    for (int key = tid; key < len; key += kAgClsThreads) {
        const float e = exp2f((s_s[key] - mx) * kLog2e);
        s_s[key] = e;
        sum += e;
        dsum = fmaf(e, dp_s[key], dsum);
    }
    sum = grad_wave_sum(sum);
    dsum = grad_wave_sum(dsum);
    if (lane == 0) {
        red[1][wave] = sum;
        red[2][wave] = dsum;
    }
    __syncthreads();
    sum = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    dsum = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    const float inv = 1.f / sum;
    const float delta = dsum * inv;
    for (int key = tid; key < len; key += kAgClsThreads) {  // (each thread revisits the keys it wrote)
        const float p = s_s[key] * inv;
        s_s[key] = (float)(_Float16)(DROP ? p * m_s[key] : p);
        dp_s[key] = (float)(_Float16)(p * (dp_s[key] - delta));
    }
    __syncthreads();
    // dK and dV rows of every key, zeros in the dQ rows behind the first
    _Float16* out = dqkv + (size_t)start * H3 + h * 64;
    for (int idx = tid; idx < len * 64; idx += kAgClsThreads) {
        const int j = idx >> 6, c = idx & 63;
        _Float16* o = out + (size_t)j * H3 + c;
        if (j > 0) o[0] = (_Float16)0.f;
        o[H] = (_Float16)(dp_s[j] * q_s[c] * 0.125f);
        o[2 * H] = (_Float16)(s_s[j] * do_s[c]);
    }
    // dQ of the first row: wave w adds keys w, w + 4, ... in key order, then the four partial sums are added in wave order
    float acc = 0.f;
    const _Float16* kcol = seq + H + lane;
    int j = wave;
    for (; j + 3 * W < len; j += 4 * W) {
        float k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) k[u] = (float)kcol[(size_t)(j + u * W) * H3];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fmaf(dp_s[j + u * W], k[u], acc);
    }
    for (; j < len; j += W) acc = fmaf(dp_s[j], (float)kcol[(size_t)j * H3], acc);
    part[wave][lane] = acc;
    __syncthreads();
    if (tid < 64) out[tid] = (_Float16)((((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]) * 0.125f);
}

// a[t][r] = X . I / 8 for swept row 16 t + 4 g + r of the chunk and owner lr: the score half of ag_tiles
__device__ __forceinline__ void ag_scores(const char* img, const ag_half8 (&x)[2], int lane, ag_f32x4 (&a)[kAgTiles]) {
    const int g = lane >> 4, lr = lane & 15;
    const int rd = lr * 128, sw0 = (g ^ (lr & 7)) << 4, sw1 = ((4 + g) ^ (lr & 7)) << 4;
#pragma unroll
    for (int t = 0; t < kAgTiles; ++t) {
        const ag_half8 i0 = *(const ag_half8*)(img + t * 2048 + rd + sw0), i1 = *(const ag_half8*)(img + t * 2048 + rd + sw1);
        ag_f32x4 s = {0.f, 0.f, 0.f, 0.f};
        s = __builtin_amdgcn_mfma_f32_16x16x32_f16(i0, x[0], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_16x16x32_f16(i1, x[1], s, 0, 0, 0);
        a[t] = s * 0.125f;
    }
    asm volatile("s_nop 7\n\ts_nop 7" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]));  // (see ag_tiles)
}

// The training forward (mdr_attention_dropout_forward, mode 0): the row pass with other operands. A workgroup owns 64 queries (Q rows in
// registers) and sweeps the keys in chunks of 64 (K and V rows staged as in attn_grad_kernel). Sweep 0 folds the chunks into a running (max, sum)
// per query: lse. Sweep 1 forms p = exp(s - lse) and Pd = p * m and accumulates ctx^T = V^T Pd^T on the staged V image. No probability goes
// to memory, and the backward recomputes lse with the same instructions. Rounding points: the list at the top of the file.
__global__ void __launch_bounds__(kAgThreads)
attn_drop_fwd_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ cu, int H, DropoutParams dpar, _Float16* __restrict__ ctx) {
    __shared__ __attribute__((aligned(128))) char img1[kAgImage];  // K rows
    __shared__ __attribute__((aligned(128))) char img2[kAgImage];  // V rows
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, lr = lane & 15;
    const int h = blockIdx.x, b = blockIdx.y, o0 = blockIdx.z * kAgOwn;
    const int start = cu[b], len = cu[b + 1] - start;
    if (o0 >= len) return;
    const size_t H3 = (size_t)3 * H;
    const _Float16* seq = qkv + (size_t)start * H3 + h * 64;
    const int owner = o0 + wave * 16 + lr;
    const bool ovalid = owner < len;
    const int orow = ovalid ? owner : len - 1;
    const bool wave_valid = o0 + wave * 16 < len;
    ag_half8 x[2];
#pragma unroll
    for (int ds = 0; ds < 2; ++ds) x[ds] = *(const ag_half8*)(seq + (size_t)orow * H3 + ds * 32 + g * 8);

    ag_f32x4 acc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] = (ag_f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f, lse = 0.f;
    const bool one_chunk = len <= kAgChunk;  // sweep 1 finds the only chunk staged

    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int c0 = 0; c0 < len; c0 += kAgChunk) {
            if (sweep == 0 || !one_chunk) {
                __syncthreads();
                ag_stage(seq + H, H3, c0, len, img1, tid);
                if (sweep == 1 || one_chunk) ag_stage(seq + 2 * H, H3, c0, len, img2, tid);
                __syncthreads();
            }
            if (!wave_valid) continue;
            ag_f32x4 s[kAgTiles];
            ag_scores(img1, x, lane, s);
            if (sweep == 0) {
                float cmax = -INFINITY;
#pragma unroll
                for (int t = 0; t < kAgTiles; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (c0 + 16 * t + 4 * g + r >= len) s[t][r] = -INFINITY;
                        cmax = fmaxf(cmax, s[t][r]);
                    }
                cmax = fmaxf(cmax, __shfl_xor(cmax, 16));
                cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
                const float m_new = fmaxf(m_run, cmax);
                const float alpha = exp2f((m_run - m_new) * kLog2e);
                const float mb = -m_new * kLog2e;
                float csum = 0.f;
#pragma unroll
                for (int t = 0; t < kAgTiles; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) csum += __builtin_amdgcn_exp2f(fmaf(s[t][r], kLog2e, mb));
                csum += __shfl_xor(csum, 16);
                csum += __shfl_xor(csum, 32);
                l_run = l_run * alpha + csum;
                m_run = m_new;
            } else {
                ag_f32x4 mk[kAgTiles], pd[kAgTiles];
                ag_mask<false>(owner, c0, g, (uint32_t)b * gridDim.x + h, dpar, mk);
#pragma unroll
                for (int t = 0; t < kAgTiles; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool live = c0 + 16 * t + 4 * g + r < len;
                        const float e = __builtin_amdgcn_exp2f((s[t][r] - lse) * kLog2e);
                        pd[t][r] = live ? e * mk[t][r] : 0.f;
                    }
                ag_accumulate(img2, pd, lane, acc);
            }
        }
        if (sweep == 0) lse = m_run + logf(l_run);
    }
    if (!ovalid) return;
    ag_store(acc, 1.f, ctx + (size_t)(start + owner) * H + h * 64, g);
}

// The training forward, mode 3: ctx is [B, H], the first query of each sequence. One workgroup per (sequence, head), shaped like
// attn_grad_cls_kernel: scores of the one query, softmax against the true maximum, fp16(p * m), then the context as four strided partial sums
// added in wave order.
__global__ void __launch_bounds__(kAgClsThreads)
attn_drop_fwd_cls_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ cu, int H, DropoutParams dpar, _Float16* __restrict__ ctx) {
    constexpr int W = kAgClsThreads / 64;
    __shared__ float q_s[64];
    __shared__ float s_s[512];  // scores, then e, then fp16(p m)
    __shared__ float red[2][W];
    __shared__ float part[W][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y;
    const int start = cu[b], len = cu[b + 1] - start;
    if (len <= 0) return;
    const size_t H3 = (size_t)3 * H;
    const _Float16* seq = qkv + (size_t)start * H3 + h * 64;
    if (tid < 64) q_s[tid] = (float)seq[tid];
    __syncthreads();
    float mx = -INFINITY;
    for (int key = tid; key < len; key += kAgClsThreads) {
        const _Float16* kp = seq + (size_t)key * H3 + H;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const ag_half8 kv = *(const ag_half8*)(kp + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) s = fmaf((float)kv[j], q_s[c * 8 + j], s);
        }
        s *= 0.125f;
        s_s[key] = s;
        mx = fmaxf(mx, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) red[0][wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    float sum = 0.f;
    for (int key = tid; key < len; key += kAgClsThreads) {
        const float e = exp2f((s_s[key] - mx) * kLog2e);
        s_s[key] = e;
        sum += e;
    }
    sum = grad_wave_sum(sum);
    if (lane == 0) red[1][wave] = sum;
    __syncthreads();
    sum = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    const float inv = 1.f / sum;
    for (int key = tid; key < len; key += kAgClsThreads)  // (each thread revisits the keys it wrote)
        s_s[key] = (float)(_Float16)(s_s[key] * inv * ag_cls_factor(key, (uint32_t)b * gridDim.x + h, dpar));
    __syncthreads();
    // wave w adds keys w, w + 4, ... in key order, then the four partial sums are added in wave order
    float acc = 0.f;
    const _Float16* vcol = seq + 2 * H + lane;
    for (int j = wave; j < len; j += W) acc = fmaf(s_s[j], (float)vcol[(size_t)j * H3], acc);
    part[wave][lane] = acc;
    __syncthreads();
    if (tid < 64) ctx[(size_t)b * H + h * 64 + tid] = (_Float16)(((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
}

bool ag_shape_ok(int B, int L, int heads, int mode) { return B >= 1 && L >= 1 && L <= 512 && heads >= 1 && heads <= 65535 && (mode == 0 || mode == 3); }

size_t ag_need(int B, int L, int heads, int mode) { return mode == 0 ? (size_t)B * L * heads * sizeof(float2) : 0; }

// what mdr_attention_backward, mdr_attention_dropout_forward and mdr_attention_dropout_backward refuse alike
int ag_check_shape(const char* fn, int B, int L, int hidden, int heads, int mode) {
    MDR_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d out of range (1..65535)", fn, B);
    MDR_REQUIRE(L >= 1 && L <= 512, "%s: L=%d out of range (1..512)", fn, L);
    MDR_REQUIRE(heads >= 1 && heads <= 65535 && hidden == 64 * heads, "%s: head dim must be 64 (hidden=%d heads=%d)", fn, hidden, heads);
    MDR_REQUIRE(mode == 0 || mode == 3, "%s: mode must be 0 (every query) or 3 (first query of each sequence), got %d", fn, mode);
    return MDR_OK;
}

// the backward's validation and launches; DROP: with the mask of `dpar` replayed
template <bool DROP>
int ag_backward(const char* fn, const void* qkv_dev, const void* dctx_dev, const int* cu_dev, int B, int L, int hidden, int heads, int mode,
                const DropoutParams& dpar, void* dqkv_dev, void* workspace_dev, size_t workspace_bytes, int device, void* stream) {
    MDR_REQUIRE(qkv_dev && dctx_dev && cu_dev && dqkv_dev, "%s: NULL pointer (qkv, dctx, cu and dqkv are required)", fn);
    if (const int rc = ag_check_shape(fn, B, L, hidden, heads, mode)) return rc;
    MDR_REQUIRE(aligned16({qkv_dev, dctx_dev, dqkv_dev, workspace_dev}), "%s: qkv, dctx, dqkv and the workspace must be 16-byte aligned", fn);
    const size_t need = ag_need(B, L, heads, mode);
    MDR_REQUIRE_WORKSPACE(fn, workspace_dev, workspace_bytes, need, "mdr_attention_backward_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    const _Float16* qkv = (const _Float16*)qkv_dev;
    const _Float16* dctx = (const _Float16*)dctx_dev;
    _Float16* dqkv = (_Float16*)dqkv_dev;
    hipStream_t st = (hipStream_t)stream;
    if (mode == 3) {
        hipLaunchKernelGGL(attn_grad_cls_kernel<DROP>, dim3(heads, B), dim3(kAgClsThreads), 0, st, qkv, dctx, cu_dev, hidden, dqkv, dpar);
        MDR_HIP_TRY(hipGetLastError());
        return MDR_OK;
    }
    // the row pass writes (lse, delta), the column pass reads them: stream order
    const dim3 grid(heads, B, (L + kAgOwn - 1) / kAgOwn);
    const size_t stat_stride = (size_t)B * L;
    hipLaunchKernelGGL((attn_grad_kernel<false, DROP>), grid, dim3(kAgThreads), 0, st, qkv, dctx, cu_dev, hidden, stat_stride, (float2*)workspace_dev, dqkv,
                       dpar);
    MDR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((attn_grad_kernel<true, DROP>), grid, dim3(kAgThreads), 0, st, qkv, dctx, cu_dev, hidden, stat_stride, (float2*)workspace_dev, dqkv,
                       dpar);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // namespace
}  // namespace mdr

extern "C" {

size_t mdr_attention_backward_workspace_bytes(int B, int L, int heads, int mode) {
    using namespace mdr;
    if (!ag_shape_ok(B, L, heads, mode)) return 0;
    return align_up(ag_need(B, L, heads, mode), 256);
}

int mdr_attention_backward(const void* qkv_dev, const void* dctx_dev, const int* cu_dev, int B, int L, int hidden, int heads, int mode, void* dqkv_dev,
                           void* workspace_dev, size_t workspace_bytes, int device, void* stream) {
    return mdr::ag_backward<false>("mdr_attention_backward", qkv_dev, dctx_dev, cu_dev, B, L, hidden, heads, mode, mdr::DropoutParams{}, dqkv_dev, workspace_dev,
                                   workspace_bytes, device, stream);
}

int mdr_attention_dropout_backward(const void* qkv_dev, const void* dctx_dev, const int* cu_dev, int B, int L, int hidden, int heads, int mode, int T,
                                   uint64_t seed, uint32_t site, void* dqkv_dev, void* workspace_dev, size_t workspace_bytes, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_attention_dropout_backward";
    MDR_REQUIRE(T >= 1 && T <= 255, "%s: T=%d out of range (1..255; without dropout the call is mdr_attention_backward)", fn, T);
    return ag_backward<true>(fn, qkv_dev, dctx_dev, cu_dev, B, L, hidden, heads, mode, dropout_params((unsigned)T, seed, site), dqkv_dev, workspace_dev,
                             workspace_bytes, device, stream);
}

int mdr_attention_dropout_forward(const void* qkv_dev, const int* cu_dev, int B, int L, int hidden, int heads, int mode, int T, uint64_t seed,
                                  uint32_t site, void* ctx_dev, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_attention_dropout_forward";
    MDR_REQUIRE(qkv_dev && cu_dev && ctx_dev, "%s: NULL pointer (qkv, cu and ctx are required)", fn);
    if (const int rc = ag_check_shape(fn, B, L, hidden, heads, mode)) return rc;
    MDR_REQUIRE(T >= 1 && T <= 255, "%s: T=%d out of range (1..255; without dropout the forward is the encoder's own)", fn, T);
    MDR_REQUIRE(aligned16({qkv_dev, ctx_dev}), "%s: qkv and ctx must be 16-byte aligned", fn);
    MDR_ENTER_DEVICE(device);
    const DropoutParams dpar = dropout_params((unsigned)T, seed, site);
    hipStream_t st = (hipStream_t)stream;
    if (mode == 3)
        hipLaunchKernelGGL(attn_drop_fwd_cls_kernel, dim3(heads, B), dim3(kAgClsThreads), 0, st, (const _Float16*)qkv_dev, cu_dev, hidden, dpar,
                           (_Float16*)ctx_dev);
    else
        hipLaunchKernelGGL(attn_drop_fwd_kernel, dim3(heads, B, (L + kAgOwn - 1) / kAgOwn), dim3(kAgThreads), 0, st, (const _Float16*)qkv_dev, cu_dev, hidden,
                           dpar, (_Float16*)ctx_dev);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // extern "C"
