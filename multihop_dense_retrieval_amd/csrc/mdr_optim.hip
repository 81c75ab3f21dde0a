// csrc/mdr_optim.hip -- the optimizer step (include/mdr_optim.h: mdr_optim_step) and the momentum encoder's EMA (mdr_optim_ema) over a table
// of parameter tensors: unscaling by the loss scale, the global-norm clip, torch.optim.Adam and the fp16 copies in one read of g and one
// read-modify-write of p, m, v, with the loss scaler's state machine on the device. No host readback, no atomics.
//
// The elements are cut into chunks of MDR_OPTIM_CHUNK = 4096, each inside one tensor (opt_chunks: a function of the sizes alone). The table
// blob holds the descriptors and, per chunk, (tensor, chunk within the tensor). A workgroup of 256 threads owns a chunk at a time: thread t
// holds the four groups of four elements (j * 256 + t) * 4 .., j = 0 .. 3, one 16-byte load each; a chunk's short tail is read and
// written element by element, so nothing behind a tensor's n is touched. The grids are capped at 2048 workgroups and stride over the chunks.
//   optim_norm_kernel      chunk c -> slot c of the workspace: {fp32 sum of (g / loss_scale)^2, some g is not finite}
//   optim_finalize_kernel  one workgroup of 1024: the slots -> grad_norm, clip_coef, mult and the loss scaler's next state
//   optim_update_kernel    Adam (<0>) or AdamW (<1>) on every element of every tensor with a g; zeroes g
//   optim_ema_kernel       k = k * m + q * (1 - m)
//
// Rounding points. Every operation is fp32 unless said otherwise, and NOTHING is contracted into an FMA (the pragma below: the kernels are
// memory-bound, and a host replay in numpy float32 gives the same bits, tests/optim_ref.py):
//   1. inv = 1 / loss_scale, once per thread; x = g * inv; x * x. Three roundings on a term's way into the sum (five counted on the square:
//      inv and x enter twice).
//   2. the thread adds its 16 squares onto 0 in element order (group j = 0 .. 3, four elements each); the xor butterfly 32, 16, .. 1 adds
//      the 64 lanes; ((w0 + w1) + w2) + w3 adds the four waves: 16 + 6 + 3 = 25 additions. A term passes through at most 30 fp32 roundings:
//      the relative error of a chunk sum, all terms being >= 0, is at most gamma_30 (gamma_k = k u / (1 - k u), u = 2^-24).
//   3. finalize: thread t of 1024 adds slots t, t + 1024, ... in order in fp64, the butterfly adds the lanes, wave sums are added in wave order:
//      fp64 throughout. grad_norm = fp32(sqrt_fp64(sum)): |grad_norm - norm| <= (gamma_30 / 2 + 2 u) norm (tests/test_optim_gpu.py).
//   4. clip_coef = min(1, max_grad_norm / (grad_norm + 1e-6f)): an add and a divide. mult = clip_coef / loss_scale: a divide, by the scale the
//      gradients carry (the scale moves afterwards). b1_pow *= beta1, b2_pow *= beta2: one multiply each per unskipped step, kept for the
//      record. The bias corrections the update uses are bias1 = 1 - beta1^k and bias2 = 1 - beta2^k, moved by
//          bias = bias + (1 - bias) * (1 - beta)        two subtractions, a multiply, an add; 1 - beta is exact for beta >= 0.5
//      so that they keep their relative precision: 1 - fp32(beta2^k) does not (fp32(0.999^k) is within 2^-25 of its value, 3e-5 of
//      1 - 0.999^k at k = 1), and a step size 1e-5 off is ten times what torch's fp32 Adam is away from fp64 after 10 steps.
//   5. update, once per thread: omb1 = 1 - beta1, omb2 = 1 - beta2, step_size = lr / bias1, bc2 = sqrt(bias2).
//      Per element:   gh = g * mult                  gd = gh + weight_decay * p          (the decay only where weight_decay != 0)
//                     m = beta1 * m + omb1 * gd      v = beta2 * v + (omb2 * gd) * gd
//                     denom = sqrt(v) / bc2 + eps    p = p - step_size * (m / denom)      p16 = fp16(p), round to nearest even
//      Divide and sqrt are the correctly rounded ones (hipcc's default for fp32).
//  5w. update with decay_mode = MDR_OPTIM_DECAY_DECOUPLED (mdr_optim_step_ex, include/mdr_optim_adamw.h): transformers.AdamW with
//      correct_bias=True as the reference's scripts/train_qa.py ran it -- as remembered, not captured: no copy of that class is at hand.
//      Once per thread: omb1 = 1 - beta1, omb2 = 1 - beta2, bc2 = sqrt(bias2), t = lr * bc2, step = t / bias1.
//      Per element, in this order:
//                     gh = g * mult                  (no decay enters gh)
//                     m = beta1 * m + omb1 * gh      v = beta2 * v + (omb2 * gh) * gh
//                     denom = sqrt(v) + eps          (eps OUTSIDE the bias correction)
//                     q = m / denom                  p = p - step * q
//                     only where weight_decay != 0:  w = lr * weight_decay      p = p - w * p     (the UPDATED p)
//                     p16 = fp16(p)
//      Norm, finalize, skip, loss scale, zero_grads and the state are mode 0's, unchanged. Mode 0 through mdr_optim_step_ex is mdr_optim_step.
//   6. EMA: mf = fp32(m), omf = fp32(1 - m) with the subtraction in double on the host; k = k * mf + q * omf; p16 = fp16(k).
// Non-finite values: the flag is the exponent test on g's bits; a non-finite sum skips as well. Nothing non-finite is used as an index.
#include <algorithm>
#include <cmath>

#include "mdr_common.h"
#include "../../include/mdr_optim.h"
#include "../../include/mdr_optim_adamw.h"

#pragma clang fp contract(off)

// MDR_OPTIM_NT: nontemporal loads and stores in the sweeps, which touch every byte once per kernel. Same bits either way. Measured on the
// RoBERTa-base list (profiles/optim_bench.md): the norm pass 0.082 ms against 0.128 ms with plain loads, the update and the EMA the same
// within 1 %, so the product build takes them; build.py -DMDR_OPTIM_NT=0 --out=... builds the plain variant for the comparison.
#ifndef MDR_OPTIM_NT
#define MDR_OPTIM_NT 1
#endif

namespace mdr {
namespace {

typedef float of32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 of16x4 __attribute__((ext_vector_type(4)));
// the table's pointers are loaded from memory: say that they point to global memory, or every access is a flat one
#define MDR_OPT_GLOBAL __attribute__((address_space(1)))
typedef MDR_OPT_GLOBAL float gf32;
typedef MDR_OPT_GLOBAL _Float16 gf16;
typedef MDR_OPT_GLOBAL of32x4 gf32x4;
typedef MDR_OPT_GLOBAL of16x4 gf16x4;

constexpr int kOptChunk = MDR_OPTIM_CHUNK;
constexpr int kOptThreads = 256;
constexpr int kOptGroups = kOptChunk / (kOptThreads * 4);  // 16-byte groups per thread and chunk
constexpr int kOptMaxGrid = 2048;
constexpr int kOptFinalThreads = 1024;
static_assert(kOptGroups * kOptThreads * 4 == kOptChunk, "a chunk is a whole number of 16-byte groups per thread");
static_assert(sizeof(mdr_optim_tensor) == 64, "the table's descriptor is 64 bytes");

struct OptSlot {
    float sum;
    int bad;
};
struct OptMap {
    int tensor, chunk;
};

template <typename T>
__device__ __forceinline__ T opt_ld(const MDR_OPT_GLOBAL T* p) {
#if MDR_OPTIM_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
template <typename T>
__device__ __forceinline__ void opt_st(MDR_OPT_GLOBAL T* p, T v) {
#if MDR_OPTIM_NT
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

__device__ __forceinline__ int opt_not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// elements of chunk `chunk` of a tensor of n elements
__device__ __forceinline__ int opt_len(int64_t n, int chunk) { return (int)min((int64_t)kOptChunk, n - (int64_t)chunk * kOptChunk); }

__global__ void __launch_bounds__(kOptThreads)
optim_norm_kernel(const mdr_optim_tensor* __restrict__ tab, const OptMap* __restrict__ map, int n_chunks, const mdr_optim_state* __restrict__ state,
                  OptSlot* __restrict__ slots) {
    __shared__ float wsum[kOptThreads / 64];
    __shared__ int wbad[kOptThreads / 64];
    const int tid = threadIdx.x;
    const float inv = 1.f / state->loss_scale;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptMap mp = map[c];
        const gf32* g = (const gf32*)tab[mp.tensor].g;
        if (!g) {  // (uniform over the workgroup)
            if (tid == 0) slots[c] = OptSlot{0.f, 0};
            continue;
        }
        const int len = opt_len(tab[mp.tensor].n, mp.chunk);
        g += (int64_t)mp.chunk * kOptChunk;
        float s = 0.f;
        int bad = 0;
        if (len == kOptChunk) {
            of32x4 gv[kOptGroups];
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j) gv[j] = opt_ld((const gf32x4*)(g + (j * kOptThreads + tid) * 4));
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float x = gv[j][i] * inv;
                    s = s + x * x;
                    bad |= opt_not_finite(gv[j][i]);
                }
        } else {
            for (int j = 0; j < kOptGroups; ++j) {
                const int e0 = (j * kOptThreads + tid) * 4;
                for (int i = 0; i < 4; ++i)
                    if (e0 + i < len) {
                        const float gi = g[e0 + i];
                        const float x = gi * inv;
                        s = s + x * x;
                        bad |= opt_not_finite(gi);
                    }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s = s + __shfl_xor(s, o);
            bad |= __shfl_xor(bad, o);
        }
        __syncthreads();  // the previous chunk's reader is done with wsum
        if ((tid & 63) == 0) {
            wsum[tid >> 6] = s;
            wbad[tid >> 6] = bad;
        }
        __syncthreads();
        if (tid == 0) slots[c] = OptSlot{((wsum[0] + wsum[1]) + wsum[2]) + wsum[3], wbad[0] | wbad[1] | wbad[2] | wbad[3]};
    }
}

__global__ void __launch_bounds__(kOptFinalThreads)
optim_finalize_kernel(const OptSlot* __restrict__ slots, int n_chunks, mdr_optim_state* state, float beta1, float beta2, float max_grad_norm, int dynamic,
                      int scale_window, float max_scale) {
    __shared__ double wsum[kOptFinalThreads / 64];
    __shared__ int wbad[kOptFinalThreads / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    int bad = 0;
    for (int c = tid; c < n_chunks; c += kOptFinalThreads) {
        const OptSlot sl = slots[c];
        s = s + (double)sl.sum;
        bad |= sl.bad;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s = s + __shfl_xor(s, o);
        bad |= __shfl_xor(bad, o);
    }
    if ((tid & 63) == 0) {
        wsum[tid >> 6] = s;
        wbad[tid >> 6] = bad;
    }
    __syncthreads();
    if (tid != 0) return;
    double total = wsum[0];
    bad = wbad[0];
    for (int w = 1; w < kOptFinalThreads / 64; ++w) {
        total = total + wsum[w];
        bad |= wbad[w];
    }
    mdr_optim_state st = *state;
    const float norm = (float)sqrt(total);
    const float coef = fminf(1.f, max_grad_norm / (norm + 1e-6f));
    st.grad_norm = norm;
    st.clip_coef = coef;
    st.mult = coef / st.loss_scale;
    if (bad || !(fabs(total) <= 1.7976931348623157e308)) {
        st.skipped_last = 1;
        st.skipped_total += 1;
        if (dynamic) {
            st.loss_scale = st.loss_scale / 2.f;
            st.unskipped = 0;
        }
    } else {
        st.skipped_last = 0;
        st.adam_step += 1;
        st.b1_pow = st.b1_pow * beta1;
        st.b2_pow = st.b2_pow * beta2;
        st.bias1 = st.bias1 + (1.f - st.bias1) * (1.f - beta1);
        st.bias2 = st.bias2 + (1.f - st.bias2) * (1.f - beta2);
        st.unskipped += 1;
        if (dynamic && st.unskipped == scale_window) {
            st.loss_scale = fminf(max_scale, 2.f * st.loss_scale);
            st.unskipped = 0;
        }
    }
    *state = st;
}

struct OptAdam {
    float mult, beta1, beta2, omb1, omb2, step_size, bc2, eps;
};

// MODE 0 (MDR_OPTIM_DECAY_L2): torch.optim.Adam, rounding point 5. MODE 1 (MDR_OPTIM_DECAY_DECOUPLED): AdamW, rounding point 5w, where
// k.step_size holds lr * sqrt(bias2) / bias1 and k.bc2 holds lr (the decay's factor is lr * weight_decay, formed per element: one multiply).
template <int MODE>
__device__ __forceinline__ void opt_adam(float g, float wd, const OptAdam& k, float& p, float& m, float& v) {
    float gd = g * k.mult;
    if constexpr (MODE == 1) {
        m = k.beta1 * m + k.omb1 * gd;
        v = k.beta2 * v + (k.omb2 * gd) * gd;
        const float denom = __builtin_sqrtf(v) + k.eps;
        p = p - k.step_size * (m / denom);
        if (wd != 0.f) p = p - (k.bc2 * wd) * p;
        return;
    }
    if (wd != 0.f) gd = gd + wd * p;
    m = k.beta1 * m + k.omb1 * gd;
    v = k.beta2 * v + (k.omb2 * gd) * gd;
    const float denom = __builtin_sqrtf(v) / k.bc2 + k.eps;
    p = p - k.step_size * (m / denom);
}

template <int MODE>
__global__ void __launch_bounds__(kOptThreads)
optim_update_kernel(const mdr_optim_tensor* __restrict__ tab, const OptMap* __restrict__ map, int n_chunks, const mdr_optim_state* __restrict__ state, float lr,
                    float beta1, float beta2, float eps, int zero_grads) {
    const int tid = threadIdx.x;
    const int skipped = state->skipped_last;
    if (skipped && !zero_grads) return;
    OptAdam k;
    k.mult = state->mult;
    k.beta1 = beta1;
    k.beta2 = beta2;
    k.omb1 = 1.f - beta1;
    k.omb2 = 1.f - beta2;
    if constexpr (MODE == 1) {
        k.step_size = (lr * __builtin_sqrtf(state->bias2)) / state->bias1;
        k.bc2 = lr;
    } else {
        k.step_size = lr / state->bias1;
        k.bc2 = __builtin_sqrtf(state->bias2);
    }
    k.eps = eps;
    const of32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptMap mp = map[c];
        const mdr_optim_tensor d = tab[mp.tensor];
        if (!d.g) continue;  // (uniform over the workgroup)
        const int len = opt_len(d.n, mp.chunk);
        const int64_t base = (int64_t)mp.chunk * kOptChunk;
        gf32* g = (gf32*)d.g + base;
        gf32* p = (gf32*)d.p + base;
        gf32* m = (gf32*)d.m + base;
        gf32* v = (gf32*)d.v + base;
        gf16* p16 = d.p16 ? (gf16*)d.p16 + base : nullptr;
        const float wd = d.weight_decay;
        if (len == kOptChunk) {
            if (skipped) {
#pragma unroll
                for (int j = 0; j < kOptGroups; ++j) opt_st((gf32x4*)(g + (j * kOptThreads + tid) * 4), zero4);
                continue;
            }
            of32x4 gv[kOptGroups], pv[kOptGroups], mv[kOptGroups], vv[kOptGroups];
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j) {
                const int e = (j * kOptThreads + tid) * 4;
                gv[j] = opt_ld((const gf32x4*)(g + e));
                pv[j] = opt_ld((const gf32x4*)(p + e));
                mv[j] = opt_ld((const gf32x4*)(m + e));
                vv[j] = opt_ld((const gf32x4*)(v + e));
            }
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j) {
                const int e = (j * kOptThreads + tid) * 4;
                float pe[4], me[4], ve[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    pe[i] = pv[j][i];
                    me[i] = mv[j][i];
                    ve[i] = vv[j][i];
                    opt_adam<MODE>(gv[j][i], wd, k, pe[i], me[i], ve[i]);
                }
                opt_st((gf32x4*)(p + e), (of32x4){pe[0], pe[1], pe[2], pe[3]});
                opt_st((gf32x4*)(m + e), (of32x4){me[0], me[1], me[2], me[3]});
                opt_st((gf32x4*)(v + e), (of32x4){ve[0], ve[1], ve[2], ve[3]});
                if (p16) opt_st((gf16x4*)(p16 + e), (of16x4){(_Float16)pe[0], (_Float16)pe[1], (_Float16)pe[2], (_Float16)pe[3]});
                if (zero_grads) opt_st((gf32x4*)(g + e), zero4);
            }
        } else {
            for (int j = 0; j < kOptGroups; ++j) {
                const int e0 = (j * kOptThreads + tid) * 4;
                for (int i = 0; i < 4; ++i) {
                    const int e = e0 + i;
                    if (e >= len) break;
                    if (!skipped) {
                        float pe = p[e], me = m[e], ve = v[e];
                        opt_adam<MODE>(g[e], wd, k, pe, me, ve);
                        p[e] = pe;
                        m[e] = me;
                        v[e] = ve;
                        if (p16) p16[e] = (_Float16)pe;
                    }
                    if (zero_grads) g[e] = 0.f;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(kOptThreads)
optim_ema_kernel(const mdr_optim_tensor* __restrict__ tab_k, const mdr_optim_tensor* __restrict__ tab_q, const OptMap* __restrict__ map, int n_chunks, float mf,
                 float omf) {
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptMap mp = map[c];
        const mdr_optim_tensor dk = tab_k[mp.tensor];
        const gf32* qp = (const gf32*)tab_q[mp.tensor].p;
        if (!dk.p || !qp) continue;  // (uniform over the workgroup)
        const int len = opt_len(min(dk.n, tab_q[mp.tensor].n), mp.chunk);  // (<= 0 behind the shorter of the two)
        const int64_t base = (int64_t)mp.chunk * kOptChunk;
        gf32* kp = (gf32*)dk.p + base;
        qp += base;
        gf16* p16 = dk.p16 ? (gf16*)dk.p16 + base : nullptr;
        if (len == kOptChunk) {
            of32x4 kv[kOptGroups], qv[kOptGroups];
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j) {
                const int e = (j * kOptThreads + tid) * 4;
                kv[j] = opt_ld((const gf32x4*)(kp + e));
                qv[j] = opt_ld((const gf32x4*)(qp + e));
            }
#pragma unroll
            for (int j = 0; j < kOptGroups; ++j) {
                const int e = (j * kOptThreads + tid) * 4;
                float r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = kv[j][i] * mf + qv[j][i] * omf;
                opt_st((gf32x4*)(kp + e), (of32x4){r[0], r[1], r[2], r[3]});
                if (p16) opt_st((gf16x4*)(p16 + e), (of16x4){(_Float16)r[0], (_Float16)r[1], (_Float16)r[2], (_Float16)r[3]});
            }
        } else {
            for (int j = 0; j < kOptGroups; ++j) {
                const int e0 = (j * kOptThreads + tid) * 4;
                for (int i = 0; i < 4; ++i) {
                    const int e = e0 + i;
                    if (e >= len) break;
                    const float r = kp[e] * mf + qp[e] * omf;
                    kp[e] = r;
                    if (p16) p16[e] = (_Float16)r;
                }
            }
        }
    }
}

__global__ void optim_state_init_kernel(mdr_optim_state* state, float loss_scale) {
    mdr_optim_state st = {};
    st.loss_scale = loss_scale;
    st.b1_pow = st.b2_pow = 1.f;
    *state = st;
}

// the number of chunks (-1: refused); first (may be NULL) gets n_tensors + 1 entries
int64_t opt_chunks(const int64_t* n, int n_tensors, int64_t* first) {
    if (!n || n_tensors < 1) return -1;
    int64_t total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (n[i] < 1) return -1;
        if (first) first[i] = total;
        total += (n[i] - 1) / kOptChunk + 1;
        if (total > 0x7fffffff) return -1;
    }
    if (first) first[n_tensors] = total;
    return total;
}

size_t opt_table_bytes(int n_tensors, int64_t chunks) { return align_up((size_t)n_tensors * sizeof(mdr_optim_tensor) + (size_t)chunks * sizeof(OptMap), 256); }

}  // namespace
}  // namespace mdr

extern "C" {

int64_t mdr_optim_chunks(const int64_t* n, int n_tensors, int64_t* first_chunk) { return mdr::opt_chunks(n, n_tensors, first_chunk); }

size_t mdr_optim_table_bytes(const int64_t* n, int n_tensors) {
    const int64_t chunks = mdr::opt_chunks(n, n_tensors, nullptr);
    return chunks < 0 ? 0 : mdr::opt_table_bytes(n_tensors, chunks);
}

size_t mdr_optim_workspace_bytes(const int64_t* n, int n_tensors) {
    const int64_t chunks = mdr::opt_chunks(n, n_tensors, nullptr);
    return chunks < 0 ? 0 : mdr::align_up((size_t)chunks * sizeof(mdr::OptSlot), 256);
}

int mdr_optim_table_fill(const mdr_optim_tensor* tensors, int n_tensors, void* table_host, size_t table_bytes, int* n_chunks) {
    using namespace mdr;
    const char* fn = "mdr_optim_table_fill";
    MDR_REQUIRE(tensors && table_host && n_chunks, "%s: NULL pointer (tensors, table_host and n_chunks are required)", fn);
    MDR_REQUIRE(n_tensors >= 1, "%s: n_tensors=%d must be at least 1", fn, n_tensors);
    int64_t total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const mdr_optim_tensor& t = tensors[i];
        MDR_REQUIRE(t.n >= 1, "%s: tensor %d has n=%lld, must be at least 1", fn, i, (long long)t.n);
        MDR_REQUIRE(t.p, "%s: tensor %d has a NULL p", fn, i);
        MDR_REQUIRE(!t.g || (t.m && t.v), "%s: tensor %d has a g but no m or v", fn, i);
        MDR_REQUIRE(aligned16({t.p, t.g, t.m, t.v}) && ((uintptr_t)t.p16 & 7) == 0,
                    "%s: tensor %d: p, g, m, v must be 16-byte aligned and p16 8-byte aligned", fn, i);
        total += (t.n - 1) / kOptChunk + 1;
        MDR_REQUIRE(total <= 0x7fffffff, "%s: more than 2^31 - 1 chunks", fn);
    }
    const size_t need = opt_table_bytes(n_tensors, total);
    MDR_REQUIRE(table_bytes >= need, "%s: table of %zu bytes, need %zu (mdr_optim_table_bytes)", fn, table_bytes, need);
    mdr_optim_tensor* out = (mdr_optim_tensor*)table_host;
    OptMap* map = (OptMap*)(out + n_tensors);
    for (int i = 0; i < n_tensors; ++i) {
        out[i] = tensors[i];
        out[i].reserved0 = 0;
        out[i].reserved1 = 0;
        const int k = (int)((tensors[i].n - 1) / kOptChunk + 1);
        for (int j = 0; j < k; ++j) *map++ = OptMap{i, j};
    }
    *n_chunks = (int)total;
    return MDR_OK;
}

int mdr_optim_state_init(mdr_optim_state* state_dev, float loss_scale, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_optim_state_init";
    MDR_REQUIRE(state_dev, "%s: NULL state", fn);
    MDR_REQUIRE(aligned16({state_dev}), "%s: state must be 16-byte aligned", fn);
    MDR_REQUIRE(loss_scale > 0.f && std::isfinite(loss_scale), "%s: loss_scale=%g must be positive and finite", fn, (double)loss_scale);
    MDR_ENTER_DEVICE(device);
    hipLaunchKernelGGL(optim_state_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state_dev, loss_scale);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int mdr_optim_step(const void* table_dev, int n_tensors, int n_chunks, mdr_optim_state* state_dev, float lr, float beta1, float beta2, float eps,
                   float max_grad_norm, int dynamic, int scale_window, float max_scale, int zero_grads, void* workspace_dev, size_t workspace_bytes,
                   int device, void* stream) {
    return mdr_optim_step_ex(table_dev, n_tensors, n_chunks, state_dev, lr, beta1, beta2, eps, max_grad_norm, dynamic, scale_window, max_scale, zero_grads,
                             MDR_OPTIM_DECAY_L2, workspace_dev, workspace_bytes, device, stream);
}

int mdr_optim_step_ex(const void* table_dev, int n_tensors, int n_chunks, mdr_optim_state* state_dev, float lr, float beta1, float beta2, float eps,
                      float max_grad_norm, int dynamic, int scale_window, float max_scale, int zero_grads, int decay_mode, void* workspace_dev,
                      size_t workspace_bytes, int device, void* stream) {
    using namespace mdr;
    const char* fn = decay_mode == MDR_OPTIM_DECAY_L2 ? "mdr_optim_step" : "mdr_optim_step_ex";
    MDR_REQUIRE(decay_mode == MDR_OPTIM_DECAY_L2 || decay_mode == MDR_OPTIM_DECAY_DECOUPLED, "%s: decay_mode must be 0 (L2, Adam) or 1 (decoupled, AdamW), got %d", fn,
                decay_mode);
    MDR_REQUIRE(table_dev && state_dev, "%s: NULL pointer (table and state are required)", fn);
    MDR_REQUIRE(n_tensors >= 1, "%s: n_tensors=%d must be at least 1", fn, n_tensors);
    MDR_REQUIRE(n_chunks >= n_tensors, "%s: n_chunks=%d is less than n_tensors=%d (mdr_optim_chunks)", fn, n_chunks, n_tensors);
    MDR_REQUIRE(aligned16({table_dev, state_dev, workspace_dev}), "%s: every pointer must be 16-byte aligned", fn);
    MDR_REQUIRE(std::isfinite(lr), "%s: lr=%g must be finite", fn, (double)lr);
    MDR_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "%s: betas (%g, %g) must lie in [0, 1)", fn, (double)beta1, (double)beta2);
    MDR_REQUIRE(eps > 0.f && std::isfinite(eps), "%s: eps=%g must be positive and finite", fn, (double)eps);
    MDR_REQUIRE(max_grad_norm > 0.f, "%s: max_grad_norm=%g must be positive", fn, (double)max_grad_norm);
    MDR_REQUIRE(dynamic == 0 || dynamic == 1, "%s: dynamic must be 0 or 1, got %d", fn, dynamic);
    MDR_REQUIRE(zero_grads == 0 || zero_grads == 1, "%s: zero_grads must be 0 or 1, got %d", fn, zero_grads);
    MDR_REQUIRE(scale_window >= 1, "%s: scale_window=%d must be at least 1", fn, scale_window);
    MDR_REQUIRE(max_scale > 0.f && std::isfinite(max_scale), "%s: max_scale=%g must be positive and finite", fn, (double)max_scale);
    const size_t need = (size_t)n_chunks * sizeof(OptSlot);
    MDR_REQUIRE_WORKSPACE(fn, workspace_dev, workspace_bytes, need, "mdr_optim_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    const mdr_optim_tensor* tab = (const mdr_optim_tensor*)table_dev;
    const OptMap* map = (const OptMap*)(tab + n_tensors);
    OptSlot* slots = (OptSlot*)workspace_dev;
    const dim3 grid(std::min(n_chunks, kOptMaxGrid));
    hipLaunchKernelGGL(optim_norm_kernel, grid, dim3(kOptThreads), 0, st, tab, map, n_chunks, state_dev, slots);
    MDR_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(kOptFinalThreads), 0, st, slots, n_chunks, state_dev, beta1, beta2, max_grad_norm, dynamic,
                       scale_window, max_scale);
    MDR_HIP_TRY(hipGetLastError());
    if (decay_mode == MDR_OPTIM_DECAY_DECOUPLED)
        hipLaunchKernelGGL(optim_update_kernel<1>, grid, dim3(kOptThreads), 0, st, tab, map, n_chunks, state_dev, lr, beta1, beta2, eps, zero_grads);
    else
        hipLaunchKernelGGL(optim_update_kernel<0>, grid, dim3(kOptThreads), 0, st, tab, map, n_chunks, state_dev, lr, beta1, beta2, eps, zero_grads);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int mdr_optim_ema(const void* table_k_dev, const void* table_q_dev, int n_tensors, int n_chunks, double m, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_optim_ema";
    MDR_REQUIRE(table_k_dev && table_q_dev, "%s: NULL pointer (both tables are required)", fn);
    MDR_REQUIRE(n_tensors >= 1, "%s: n_tensors=%d must be at least 1", fn, n_tensors);
    MDR_REQUIRE(n_chunks >= n_tensors, "%s: n_chunks=%d is less than n_tensors=%d (mdr_optim_chunks)", fn, n_chunks, n_tensors);
    MDR_REQUIRE(aligned16({table_k_dev, table_q_dev}), "%s: every pointer must be 16-byte aligned", fn);
    MDR_REQUIRE(m >= 0.0 && m <= 1.0, "%s: m=%g must lie in [0, 1]", fn, m);
    MDR_ENTER_DEVICE(device);
    const mdr_optim_tensor* tk = (const mdr_optim_tensor*)table_k_dev;
    hipLaunchKernelGGL(optim_ema_kernel, dim3(std::min(n_chunks, kOptMaxGrid)), dim3(kOptThreads), 0, (hipStream_t)stream, tk,
                       (const mdr_optim_tensor*)table_q_dev, (const OptMap*)(tk + n_tensors), n_chunks, (float)m, (float)(1.0 - m));
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // extern "C"
