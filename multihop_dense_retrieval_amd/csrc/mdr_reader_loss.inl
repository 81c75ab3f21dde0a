// csrc/mdr_reader_loss.inl -- the answer reader's training loss and its three heads with gradients (include/mdr_reader_loss.h). Included at
// the end of mdr_reader.inl: the heads' forward is that file's reader_logits / reader_rank / reader_sp kernels, launched here on caller-given
// tensors, so the training forward's bits are the inference forward's by construction. Not a translation unit of its own.
//
// Replaces mdr/qa/qa_model.py:73-102 of the reference (the training branch of QAModel.forward) and the backward of :59-69.
//
// Kernels
//   reader_loss_row      one workgroup per row b: the two logit rows in LDS, lse_s and lse_e (wave reductions), the A candidates walked by the
//                        workgroup (thread t takes a = t, t + 256, ..), M_b, the row's rank BCE and sp BCE sum -> part[3][B]
//   reader_loss_total    one wave: the three sums over b (lane l adds b = l, l + 64, .. in order, then the butterfly), the total
//   reader_loss_grad     one workgroup per row: lse and M_b again (the same code, the same bits), then per tile of 256 candidates the (s, e, p)
//                        triples go through LDS and thread t adds, in candidate order, the p of those that name its positions t and t + 256
//   reader_heads_token_grad   a workgroup owns a chunk of the padded (b, p) index space, a wave a token row at a time: reads the h16 row, writes
//                        the d_h row, keeps the partial dw_start / dw_end / dw_sp in registers; the four waves are added in order into
//                        part[S][3][H], then grad_strand_reduce_kernel (csrc/mdr_grad_common.h)
//   reader_heads_bias_grad    one workgroup: db_qa and db_sp as ordered sums
//   reader_rank_grad     a thread owns column e of d_dense16 and dw_rank and walks b in order
// Every output element has one owner and one summation order: no atomics, and two runs give the same bits.
//
// Rounding points (apex O1 as remembered, not captured; tests/reader_loss_ref.py states them in fp64 and derives its bound from this list):
//   loss   1. logits, rank and sp scores are fp16, widened exactly; everything else is fp32 (expf / logf / log1pf of the device library).
//          2. lse = m + log(sum of exp(x - m)) over the entries that are not -inf, m their maximum; ls = lse - x[s]; log_prob = -(ls + le);
//             p = exp(log_prob), 0 if log_prob == 0; M = sum p; the row's loss is -log M.
//          3. bce(x, y) = max(x, 0) - x y + log1p(exp(-|x|)); the sp term is (bce * float(offset)) * float(label).
//          4. loss = (rank_sum + span_sum) + sp_weight * sp_sum: never rounded to fp16.
//   grads  5. d_start = fp16( (g0 / M) * (exp(x - lse) * P_s - hit_s[l]) ), P_s = sum of p over the candidates whose start is not ignored,
//             hit_s[l] the sum of p over those with s_a = l; one rounding to fp16. d_end likewise.
//          6. d_rank = fp16( g0 * (sigmoid(x) - y) ), d_sp = fp16( (((g0 * sp_weight) * offset) * label) * (sigmoid(x) - y) ).
//   heads  7. forward: the rounding points listed at the top of mdr_reader.inl.
//          8. d_h = fp16( fma(g_sp, w_sp, fma(g_e, w_e, g_s * w_s)) ) with fp16 operands widened: three fp32 roundings, one fp16 rounding;
//             g_sp of a row is the fp32 sum, in j order, of the fp16 gradients whose offset names it.
//          9. dw rows: fp32 fma chains over the token rows of a chunk, the four waves added in order, the chunks by the strand reduce.
//         10. pooled16 = fp16(tanh(dense16)); d_pooled = fp16(g_rank * w_rank); d_dense16 = fp16(d_pooled * (1 - pooled16^2)), the factor
//             formed in fp32 by one fma; dw_rank = fp32 fma chain over b of g_rank * pooled16.
#include "../../include/mdr_reader_loss.h"
#include "mdr_grad_common.h"

namespace mdr {
namespace {

constexpr int kRlThreads = 256;
constexpr int kRlMaxL = kSpanMaxL;  // two rows of fp32 in LDS
constexpr int kRhSteps = kGradMaxH / 128;  // half2 steps of a lane over one row

__device__ __forceinline__ float rl_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// the sum (or maximum) over the workgroup's 256 threads: the butterfly inside a wave, the four waves in order; every thread gets it
template <bool MAX>
__device__ __forceinline__ float rl_block_reduce(float v, float* red) {
    v = MAX ? rl_wave_max(v) : grad_wave_sum(v);
    __syncthreads();  // the previous use of red is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return MAX ? fmaxf(fmaxf(fmaxf(red[0], red[1]), red[2]), red[3]) : ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ float rl_row_lse(const float* x, int L, float* red) {
    float m = -INFINITY;
    for (int p = threadIdx.x; p < L; p += kRlThreads) m = fmaxf(m, x[p]);
    m = rl_block_reduce<true>(m, red);
    float s = 0.f;
    for (int p = threadIdx.x; p < L; p += kRlThreads)
        if (x[p] != -INFINITY) s += expf(x[p] - m);
    s = rl_block_reduce<false>(s, red);
    return m + logf(s);
}

// exp(log_prob) of one candidate, 0 for a masked one; si / ei: its positions, -1 where ignored
__device__ __forceinline__ float rl_candidate(const float* st, const float* en, int L, float lse_s, float lse_e, long long s, long long e, int& si, int& ei) {
    si = s >= 0 && s < L ? (int)s : -1;
    ei = e >= 0 && e < L ? (int)e : -1;
    const float ls = si >= 0 ? lse_s - st[si] : 0.f;
    const float le = ei >= 0 ? lse_e - en[ei] : 0.f;
    const float lp = -(ls + le);
    return lp == 0.f ? 0.f : expf(lp);
}

__device__ __forceinline__ float rl_bce(float x, float y) { return fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float rl_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ void rl_stage_rows(const unsigned short* start, const unsigned short* end, int b, int L, float* st, float* en) {
    for (int p = threadIdx.x; p < L; p += kRlThreads) {
        st[p] = h16_bits_to_f(start[(size_t)b * L + p]);
        en[p] = h16_bits_to_f(end[(size_t)b * L + p]);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kRlThreads)
reader_loss_row_kernel(const unsigned short* __restrict__ start, const unsigned short* __restrict__ end, const unsigned short* __restrict__ rank,
                       const unsigned short* __restrict__ sp, const long long* __restrict__ starts, const long long* __restrict__ ends,
                       const long long* __restrict__ label, const long long* __restrict__ offs, const long long* __restrict__ slab, int B, int L, int A,
                       int NS, float* __restrict__ part) {
    __shared__ float st[kRlMaxL], en[kRlMaxL];
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    rl_stage_rows(start, end, b, L, st, en);
    const float lse_s = rl_row_lse(st, L, red), lse_e = rl_row_lse(en, L, red);
    float m = 0.f;
    for (int a = tid; a < A; a += kRlThreads) {
        int si, ei;
        m += rl_candidate(st, en, L, lse_s, lse_e, starts[(size_t)b * A + a], ends[(size_t)b * A + a], si, ei);
    }
    m = rl_block_reduce<false>(m, red);
    const float y = (float)label[b];
    float spl = 0.f;
    if (sp)
        for (int j = tid; j < NS; j += kRlThreads) {
            const size_t i = (size_t)b * NS + j;
            spl += (rl_bce(h16_bits_to_f(sp[i]), (float)slab[i]) * (float)offs[i]) * y;
        }
    spl = rl_block_reduce<false>(spl, red);
    if (tid == 0) {
        part[b] = m != 0.f ? -logf(m) : 0.f;
        part[B + b] = rl_bce(h16_bits_to_f(rank[b]), y);
        part[2 * B + b] = spl;
    }
}

__global__ void __launch_bounds__(64)
reader_loss_total_kernel(const float* __restrict__ part, int B, float sp_weight, int has_sp, float* __restrict__ loss) {
    float s[3] = {0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < B; b += 64) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += part[k * B + b];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = grad_wave_sum(s[k]);
    if (threadIdx.x == 0) {
        float t = s[1] + s[0];
        if (has_sp) t += s[2] * sp_weight;
        loss[0] = t;
    }
}

__global__ void __launch_bounds__(kRlThreads)
reader_loss_grad_kernel(const unsigned short* __restrict__ start, const unsigned short* __restrict__ end, const unsigned short* __restrict__ rank,
                        const unsigned short* __restrict__ sp, const long long* __restrict__ starts, const long long* __restrict__ ends,
                        const long long* __restrict__ label, const long long* __restrict__ offs, const long long* __restrict__ slab, int B, int L, int A,
                        int NS, float sp_weight, const float* __restrict__ g0p, unsigned short* __restrict__ d_start, unsigned short* __restrict__ d_end,
                        unsigned short* __restrict__ d_rank, unsigned short* __restrict__ d_sp) {
    __shared__ float st[kRlMaxL], en[kRlMaxL];
    __shared__ float red[4];
    __shared__ int ts[kRlThreads], te[kRlThreads];
    __shared__ float tp[kRlThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    rl_stage_rows(start, end, b, L, st, en);
    const float lse_s = rl_row_lse(st, L, red), lse_e = rl_row_lse(en, L, red);
    float m = 0.f, ps = 0.f, pe = 0.f;
    float hs[2] = {0.f, 0.f}, he[2] = {0.f, 0.f};  // positions tid and tid + 256
    for (int a0 = 0; a0 < A; a0 += kRlThreads) {
        const int a = a0 + tid;
        int si = -1, ei = -1;
        float p = 0.f;
        if (a < A) p = rl_candidate(st, en, L, lse_s, lse_e, starts[(size_t)b * A + a], ends[(size_t)b * A + a], si, ei);
        m += p;
        if (si >= 0) ps += p;
        if (ei >= 0) pe += p;
        ts[tid] = si;
        te[tid] = ei;
        tp[tid] = p;
        __syncthreads();
        const int n = min(kRlThreads, A - a0);
        for (int k = 0; k < n; ++k) {
            const int s = ts[k], e = te[k];
            const float p_k = tp[k];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (s == tid + r * kRlThreads) hs[r] += p_k;
                if (e == tid + r * kRlThreads) he[r] += p_k;
            }
        }
        __syncthreads();
    }
    m = rl_block_reduce<false>(m, red);
    ps = rl_block_reduce<false>(ps, red);
    pe = rl_block_reduce<false>(pe, red);
    const float g0 = g0p[0];
    const bool counted = m != 0.f;
    const float coef = g0 / m;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int l = tid + r * kRlThreads;
        if (l < L) {
            const float xs = st[l], xe = en[l];
            const float ds = counted && xs != -INFINITY ? coef * (expf(xs - lse_s) * ps - hs[r]) : 0.f;
            const float de = counted && xe != -INFINITY ? coef * (expf(xe - lse_e) * pe - he[r]) : 0.f;
            d_start[(size_t)b * L + l] = f_to_h16_bits(ds);
            d_end[(size_t)b * L + l] = f_to_h16_bits(de);
        }
    }
    const float y = (float)label[b];
    if (tid == 0) d_rank[b] = f_to_h16_bits(g0 * (rl_sigmoid(h16_bits_to_f(rank[b])) - y));
    if (sp && d_sp)
        for (int j = tid; j < NS; j += kRlThreads) {
            const size_t i = (size_t)b * NS + j;
            const float wgt = ((g0 * sp_weight) * (float)offs[i]) * y;
            d_sp[i] = f_to_h16_bits(wgt * (rl_sigmoid(h16_bits_to_f(sp[i])) - (float)slab[i]));
        }
}

// ------------------------------------------------------------------------------------------------------------------------ the heads' backward
// grid S, chunk c owns the padded indices [c rpc, (c + 1) rpc) of [B, L]; part [S][3][H]: dw_start, dw_end, dw_sp
__global__ void __launch_bounds__(256)
reader_heads_token_grad_kernel(const _Float16* __restrict__ h, const int* __restrict__ cu, const long long* __restrict__ pmask,
                               const long long* __restrict__ offs, int B, int L, int NS, int H, int rows_cap, int rpc, const _Float16* __restrict__ w,
                               const unsigned short* __restrict__ gs16, const unsigned short* __restrict__ ge16, const unsigned short* __restrict__ gsp16,
                               _Float16* __restrict__ dh, float* __restrict__ part) {
    typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
    __shared__ float red[4][3 * kGradMaxH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = H >> 7;
    half2_t w0[kRhSteps], w1[kRhSteps], w2[kRhSteps];
    float a0[2 * kRhSteps], a1[2 * kRhSteps], a2[2 * kRhSteps];
#pragma unroll
    for (int k = 0; k < kRhSteps; ++k) {
        a0[2 * k] = a0[2 * k + 1] = a1[2 * k] = a1[2 * k + 1] = a2[2 * k] = a2[2 * k + 1] = 0.f;
        if (k < n) {
            const int e = 2 * lane + 128 * k;
            w0[k] = *(const half2_t*)(w + e);
            w1[k] = *(const half2_t*)(w + H + e);
            w2[k] = *(const half2_t*)(w + 3 * (size_t)H + e);
        }
    }
    const int total = min(cu[B], rows_cap);
    const long long i_end = min((long long)(blockIdx.x + 1) * rpc, (long long)B * L);
    for (long long i = (long long)blockIdx.x * rpc + wave; i < i_end; i += 4) {
        const int b = (int)(i / L), p = (int)(i - (long long)b * L);
        const int c0 = cu[b], len = cu[b + 1] - c0;
        if (p >= len) continue;
        const int t = c0 + p;
        if (t < 0 || t >= total) continue;
        float gs = 0.f, ge = 0.f, gp = 0.f;
        if (pmask[i] == 1) {
            gs = h16_bits_to_f(gs16[i]);
            ge = h16_bits_to_f(ge16[i]);
        }
        if (gsp16)
            for (int j = 0; j < NS; ++j)
                if (offs[(size_t)b * NS + j] == p) gp += h16_bits_to_f(gsp16[(size_t)b * NS + j]);
        const bool any = gs != 0.f || ge != 0.f || gp != 0.f;  // (uniform over the wave) a row no head reads: zeros, and h is not read
        const _Float16* x = h + (size_t)t * H;
        _Float16* o = dh + (size_t)t * H;
#pragma unroll
        for (int k = 0; k < kRhSteps; ++k)
            if (k < n) {
                const int e = 2 * lane + 128 * k;
                half2_t d = {(_Float16)0.f, (_Float16)0.f};
                if (any) {
                    const half2_t xv = *(const half2_t*)(x + e);
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        d[c] = (_Float16)__builtin_fmaf(gp, (float)w2[k][c], __builtin_fmaf(ge, (float)w1[k][c], gs * (float)w0[k][c]));
                        a0[2 * k + c] = __builtin_fmaf(gs, (float)xv[c], a0[2 * k + c]);
                        a1[2 * k + c] = __builtin_fmaf(ge, (float)xv[c], a1[2 * k + c]);
                        a2[2 * k + c] = __builtin_fmaf(gp, (float)xv[c], a2[2 * k + c]);
                    }
                }
                *(half2_t*)(o + e) = d;
            }
    }
#pragma unroll
    for (int k = 0; k < kRhSteps; ++k)
        if (k < n) {
            const int e = 2 * lane + 128 * k;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                red[wave][e + c] = a0[2 * k + c];
                red[wave][H + e + c] = a1[2 * k + c];
                red[wave][2 * H + e + c] = a2[2 * k + c];
            }
        }
    __syncthreads();
    for (int e = tid; e < 3 * H; e += 256) part[(size_t)blockIdx.x * 3 * H + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

// one workgroup: db_qa[0] = sum g_s, db_qa[1] = sum g_e over the positions the forward did not mask; db_sp = sum g_sp over the offsets inside their row
__global__ void __launch_bounds__(kRlThreads)
reader_heads_bias_grad_kernel(const int* __restrict__ cu, const long long* __restrict__ pmask, const long long* __restrict__ offs, int B, int L, int NS,
                              const unsigned short* __restrict__ gs16, const unsigned short* __restrict__ ge16, const unsigned short* __restrict__ gsp16,
                              float* __restrict__ db_qa, float* __restrict__ db_sp, int accumulate) {
    __shared__ float red[4];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    const long long n = (long long)B * L;
    for (long long i = threadIdx.x; i < n; i += kRlThreads) {
        const int b = (int)(i / L), p = (int)(i - (long long)b * L);
        if (p < cu[b + 1] - cu[b] && pmask[i] == 1) {
            s0 += h16_bits_to_f(gs16[i]);
            s1 += h16_bits_to_f(ge16[i]);
        }
    }
    if (gsp16)
        for (int i = threadIdx.x; i < B * NS; i += kRlThreads) {
            const int b = i / NS;
            const long long p = offs[i];
            if (p >= 0 && p < cu[b + 1] - cu[b]) s2 += h16_bits_to_f(gsp16[i]);
        }
    s0 = rl_block_reduce<false>(s0, red);
    s1 = rl_block_reduce<false>(s1, red);
    s2 = rl_block_reduce<false>(s2, red);
    if (threadIdx.x == 0) {
        db_qa[0] = accumulate ? s0 + db_qa[0] : s0;
        db_qa[1] = accumulate ? s1 + db_qa[1] : s1;
        if (db_sp) db_sp[0] = accumulate ? s2 + db_sp[0] : s2;
    }
}

// grid H / 64, 64 threads: thread e walks b = 0 .. B - 1
__global__ void __launch_bounds__(64)
reader_rank_grad_kernel(const _Float16* __restrict__ dense, int B, int H, const _Float16* __restrict__ w, const unsigned short* __restrict__ g16,
                        _Float16* __restrict__ d_dense, float* __restrict__ dw, float* __restrict__ db, int accumulate) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    const float wv = (float)w[e];
    float acc = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
        const float g = h16_bits_to_f(g16[b]);
        const float pooled = (float)(_Float16)tanhf((float)dense[(size_t)b * H + e]);
        const float dp = (float)(_Float16)(g * wv);
        d_dense[(size_t)b * H + e] = (_Float16)(dp * __builtin_fmaf(-pooled, pooled, 1.f));
        acc = __builtin_fmaf(g, pooled, acc);
        sb += g;
    }
    dw[e] = accumulate ? acc + dw[e] : acc;
    if (e == 0) db[0] = accumulate ? sb + db[0] : sb;
}

bool rl_loss_shape_ok(int B, int L, int A, int NS) { return B >= 1 && L >= 1 && L <= kRlMaxL && A >= 1 && NS >= 0; }
bool rh_shape_ok(int B, int L, int NS, int H) {
    return B >= 1 && L >= 1 && NS >= 0 && H >= 128 && H <= kGradMaxH && H % 128 == 0 && (long long)B * L < (1ll << 31) && (long long)B * (NS > 0 ? NS : 1) < (1ll << 31);
}

}  // namespace
}  // namespace mdr

extern "C" {

size_t mdr_reader_loss_workspace_bytes(int batch, int seq_len, int n_cand, int n_sent) {
    if (!rl_loss_shape_ok(batch, seq_len, n_cand, n_sent)) return 0;
    return align_up((size_t)3 * batch * sizeof(float), 256);
}

#define MDR_RL_REQUIRE_INPUTS(fn)                                                                                                                  \
    MDR_REQUIRE(rl_loss_shape_ok(batch, seq_len, n_cand, n_sent), "%s: bad shape batch=%d seq_len=%d n_cand=%d n_sent=%d (1 <= seq_len <= %d)", fn, \
                batch, seq_len, n_cand, n_sent, kRlMaxL);                                                                                         \
    MDR_REQUIRE(start_logits_dev && end_logits_dev && rank_score_dev && starts_dev && ends_dev && label_dev, "%s: NULL input pointer", fn);        \
    MDR_REQUIRE(!(sp_score_dev && n_sent > 0) || (sent_offsets_dev && sent_labels_dev), "%s: sp_score given without sent_offsets / sent_labels", fn)

int mdr_reader_loss_forward(const uint16_t* start_logits_dev, const uint16_t* end_logits_dev, const uint16_t* rank_score_dev,
                            const uint16_t* sp_score_dev, const int64_t* starts_dev, const int64_t* ends_dev, const int64_t* label_dev,
                            const int64_t* sent_offsets_dev, const int64_t* sent_labels_dev, int batch, int seq_len, int n_cand, int n_sent,
                            float sp_weight, float* loss_dev, void* workspace_dev, size_t workspace_bytes, int device, void* stream) {
    const char* fn = "mdr_reader_loss_forward";
    MDR_RL_REQUIRE_INPUTS(fn);
    MDR_REQUIRE(loss_dev != nullptr, "%s: NULL output pointer", fn);
    MDR_REQUIRE(aligned16({workspace_dev}), "%s: the workspace must be 16-byte aligned", fn);
    const size_t need = align_up((size_t)3 * batch * sizeof(float), 256);
    MDR_REQUIRE_WORKSPACE(fn, workspace_dev, workspace_bytes, need, "mdr_reader_loss_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace_dev;
    hipLaunchKernelGGL(reader_loss_row_kernel, dim3(batch), dim3(kRlThreads), 0, st, start_logits_dev, end_logits_dev, rank_score_dev, sp_score_dev,
                       (const long long*)starts_dev, (const long long*)ends_dev, (const long long*)label_dev, (const long long*)sent_offsets_dev,
                       (const long long*)sent_labels_dev, batch, seq_len, n_cand, n_sent, part);
    MDR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(reader_loss_total_kernel, dim3(1), dim3(64), 0, st, (const float*)part, batch, sp_weight, sp_score_dev ? 1 : 0, loss_dev);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int mdr_reader_loss_backward(const uint16_t* start_logits_dev, const uint16_t* end_logits_dev, const uint16_t* rank_score_dev,
                             const uint16_t* sp_score_dev, const int64_t* starts_dev, const int64_t* ends_dev, const int64_t* label_dev,
                             const int64_t* sent_offsets_dev, const int64_t* sent_labels_dev, int batch, int seq_len, int n_cand, int n_sent,
                             float sp_weight, const float* g0_dev, uint16_t* d_start_dev, uint16_t* d_end_dev, uint16_t* d_rank_dev,
                             uint16_t* d_sp_dev, int device, void* stream) {
    const char* fn = "mdr_reader_loss_backward";
    MDR_RL_REQUIRE_INPUTS(fn);
    MDR_REQUIRE(g0_dev && d_start_dev && d_end_dev && d_rank_dev, "%s: NULL pointer (g0, d_start, d_end and d_rank are required)", fn);
    MDR_REQUIRE(!(sp_score_dev && n_sent > 0) || d_sp_dev, "%s: sp_score given without d_sp", fn);
    MDR_ENTER_DEVICE(device);
    hipLaunchKernelGGL(reader_loss_grad_kernel, dim3(batch), dim3(kRlThreads), 0, (hipStream_t)stream, start_logits_dev, end_logits_dev, rank_score_dev,
                       sp_score_dev, (const long long*)starts_dev, (const long long*)ends_dev, (const long long*)label_dev,
                       (const long long*)sent_offsets_dev, (const long long*)sent_labels_dev, batch, seq_len, n_cand, n_sent, sp_weight, g0_dev, d_start_dev,
                       d_end_dev, d_rank_dev, d_sp_dev);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

#define MDR_RH_REQUIRE_INPUTS(fn)                                                                                                             \
    MDR_REQUIRE(rh_shape_ok(batch, seq_len, n_sent, hidden), "%s: bad shape batch=%d seq_len=%d n_sent=%d hidden=%d (hidden: a multiple of 128, 128 .. %d)", \
                fn, batch, seq_len, n_sent, hidden, kGradMaxH);                                                                               \
    MDR_REQUIRE(h16_dev && cu_dev && dense16_dev && paragraph_mask_dev && w_head16_dev, "%s: NULL input pointer", fn);                         \
    MDR_REQUIRE(aligned16({h16_dev, dense16_dev, w_head16_dev}), "%s: h16, dense16 and w_head16 must be 16-byte aligned", fn)

int mdr_reader_heads_forward(const void* h16_dev, const int* cu_dev, const void* dense16_dev, const int64_t* paragraph_mask_dev,
                             const int64_t* sent_offsets_dev, int batch, int seq_len, int n_sent, int hidden, const void* w_head16_dev,
                             const float* b_head_dev, uint16_t* start_logits_dev, uint16_t* end_logits_dev, uint16_t* rank_score_dev,
                             uint16_t* sp_score_dev, int device, void* stream) {
    const char* fn = "mdr_reader_heads_forward";
    MDR_RH_REQUIRE_INPUTS(fn);
    MDR_REQUIRE(b_head_dev && start_logits_dev && end_logits_dev && rank_score_dev, "%s: NULL pointer (b_head and the three outputs are required)", fn);
    const bool has_sp = sp_score_dev && n_sent > 0;
    MDR_REQUIRE(!has_sp || sent_offsets_dev, "%s: sp_score given without sent_offsets", fn);
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const int B = batch, L = seq_len, H = hidden;
    const _Float16* w = (const _Float16*)w_head16_dev;
    hipLaunchKernelGGL(reader_logits_kernel, dim3((B * L + 3) / 4), dim3(256), 0, st, (const _Float16*)h16_dev, cu_dev, (const long long*)paragraph_mask_dev,
                       B, L, H, w, b_head_dev, start_logits_dev, end_logits_dev);
    hipLaunchKernelGGL(reader_rank_kernel, dim3((B + 3) / 4), dim3(256), 0, st, (const _Float16*)dense16_dev, B, H, w + (size_t)2 * H, b_head_dev + 2,
                       rank_score_dev);
    if (has_sp)
        hipLaunchKernelGGL(reader_sp_kernel, dim3((B * n_sent + 3) / 4), dim3(256), 0, st, (const _Float16*)h16_dev, cu_dev,
                           (const long long*)sent_offsets_dev, B, L, n_sent, H, w + (size_t)3 * H, b_head_dev + 3, sp_score_dev, (unsigned short*)nullptr);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

size_t mdr_reader_heads_backward_workspace_bytes(int batch, int seq_len, int hidden) {
    if (!rh_shape_ok(batch, seq_len, 0, hidden)) return 0;
    int rpc;
    const int S = grad_row_chunks(batch * seq_len, hidden, 3, &rpc);
    return align_up((size_t)S * 3 * hidden * sizeof(float), 256);
}

int mdr_reader_heads_backward(const void* h16_dev, const int* cu_dev, const void* dense16_dev, const int64_t* paragraph_mask_dev,
                              const int64_t* sent_offsets_dev, int batch, int seq_len, int n_sent, int hidden, int rows_cap,
                              const void* w_head16_dev, const uint16_t* g_start_dev, const uint16_t* g_end_dev, const uint16_t* g_rank_dev,
                              const uint16_t* g_sp_dev, void* d_h16_dev, void* d_dense16_dev, float* dw_qa_dev, float* db_qa_dev,
                              float* dw_sp_dev, float* db_sp_dev, float* dw_rank_dev, float* db_rank_dev, int accumulate, void* workspace_dev,
                              size_t workspace_bytes, int device, void* stream) {
    const char* fn = "mdr_reader_heads_backward";
    MDR_RH_REQUIRE_INPUTS(fn);
    MDR_REQUIRE(rows_cap >= 1, "%s: rows_cap=%d must be at least 1", fn, rows_cap);
    MDR_REQUIRE(g_start_dev && g_end_dev && g_rank_dev, "%s: NULL gradient pointer (g_start, g_end and g_rank are required)", fn);
    MDR_REQUIRE(d_h16_dev && d_dense16_dev && dw_qa_dev && db_qa_dev && dw_rank_dev && db_rank_dev, "%s: NULL output pointer", fn);
    const bool has_sp = g_sp_dev && n_sent > 0;
    MDR_REQUIRE(!has_sp || (sent_offsets_dev && dw_sp_dev && db_sp_dev), "%s: g_sp given without sent_offsets, dw_sp or db_sp", fn);
    MDR_REQUIRE(aligned16({d_h16_dev, d_dense16_dev, dw_qa_dev, dw_sp_dev, dw_rank_dev, workspace_dev}),
                "%s: d_h16, d_dense16, dw_qa, dw_sp, dw_rank and the workspace must be 16-byte aligned", fn);
    const int B = batch, L = seq_len, H = hidden;
    int rpc;
    const int S = grad_row_chunks(B * L, H, 3, &rpc);
    const size_t need = align_up((size_t)S * 3 * H * sizeof(float), 256);
    MDR_REQUIRE_WORKSPACE(fn, workspace_dev, workspace_bytes, need, "mdr_reader_heads_backward_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const _Float16* w = (const _Float16*)w_head16_dev;
    const int acc = accumulate ? 1 : 0;
    float* part = (float*)workspace_dev;
    hipLaunchKernelGGL(reader_heads_token_grad_kernel, dim3(S), dim3(256), 0, st, (const _Float16*)h16_dev, cu_dev, (const long long*)paragraph_mask_dev,
                       (const long long*)sent_offsets_dev, B, L, n_sent, H, rows_cap, rpc, w, g_start_dev, g_end_dev, has_sp ? g_sp_dev : (const uint16_t*)nullptr,
                       (_Float16*)d_h16_dev, part);
    MDR_HIP_TRY(hipGetLastError());
    if (int rc = launch_strand_reduce(part, S, 3, H, dw_qa_dev, dw_qa_dev + H, has_sp ? dw_sp_dev : nullptr, acc, st)) return rc;
    hipLaunchKernelGGL(reader_heads_bias_grad_kernel, dim3(1), dim3(kRlThreads), 0, st, cu_dev, (const long long*)paragraph_mask_dev,
                       (const long long*)sent_offsets_dev, B, L, n_sent, g_start_dev, g_end_dev, has_sp ? g_sp_dev : (const uint16_t*)nullptr, db_qa_dev,
                       has_sp ? db_sp_dev : (float*)nullptr, acc);
    hipLaunchKernelGGL(reader_rank_grad_kernel, dim3(H / 64), dim3(64), 0, st, (const _Float16*)dense16_dev, B, H, w + (size_t)2 * H, g_rank_dev,
                       (_Float16*)d_dense16_dev, dw_rank_dev, db_rank_dev, acc);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

#undef MDR_RL_REQUIRE_INPUTS
#undef MDR_RH_REQUIRE_INPUTS

}  // extern "C"
