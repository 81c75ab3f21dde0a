// csrc/mdr_layernorm_grad.hip -- the backward of a LayerNorm of the trunk on packed rows (include/mdr_layernorm_grad.h:
// mdr_layernorm_backward) and of the CLS gather (mdr_gather_cls_backward). The forward is layernorm_kernel of csrc/mdr_encoder_pack_ln.inl,
//     y = (x - mu) * rstd * g + b,   x = in (+ res16 | res32),
// and it saves nothing: the backward recomputes x, mu and rstd from the same inputs. Per row, with dy = fp32(dy16) + fp32(dy2):
//     xhat = (x - mu) * rstd    a = dy * g    c1 = mean(a)    c2 = mean(a * xhat)    dx = rstd * (a - c1 - xhat * c2)
//     dg = sum over rows of dy * xhat          db = sum over rows of dy
//
// ln_grad_kernel<IN_T, NV>: the rows are cut into S chunks of rows_per_chunk rows (grad_row_chunks: a function of (M, H) alone). One workgroup
//   of four waves owns a chunk. A wave owns a row, as in the forward, with the forward's element order per lane: H % 256 == 0 (NV = H / 256,
//   a compile-time count that keeps the registers of H = 768 at three groups) lane l holds the NV groups of four columns (l + 64 i) * 4 ..,
//   one 16-byte load per fp32 group; otherwise (NV = 0) the H / 64 columns l + 64 i. Wave w
//   walks rows w, w + 4, ... of the chunk in order, writes dx of each row and keeps its lanes' dg and db columns in registers. The four
//   waves' columns are added through LDS in wave order. S = 1: the workgroup writes dg and db itself (+ the old value). Otherwise it
//   writes its sums to the workspace [S][2][H], and grad_strand_reduce_kernel adds them in a fixed order: strand j of sixteen adds chunks j,
//   j + 16, ... in order (sixteen times the loads in flight of one chain over up to 1024 chunks), the min(S, 16) strands are added in strand
//   order, then the old value. A chunk at or behind the valid count writes zeros. Every output element has one owner and one summation order: no atomics, two runs give the same bits.
// grad_strand_reduce_kernel is defined here once and serves the embedding backward too (launch_strand_reduce of csrc/mdr_grad_common.h).
// gather_cls_grad_kernel: one thread per element of d16 [B, H]; row cu[b] of acc16 has one owner.
//
// Rounding points (tests/layernorm_grad_ref.py derives its bound from this list; every operation is fp32, and a multiply feeding an add may
// be fused or not):
//   1. x = fp32(in) + fp32(residual): one rounded add, none without a residual. The forward's expression.
//   2. mu = wave_sum(s) / H: s adds the lane's elements in index order (VEC: ((x0 + x1) + x2) + x3 per group, then onto s), wave_sum is the
//      xor butterfly 32, 16, .. 1; var the same over (x - mu)^2 in element order; rstd = rsqrtf(var / H + eps). The forward's expressions
//      in the forward's order.
//   3. dy = fp32(dy16) + fp32(dy2): one rounded add, none when only one is given.
//   4. xhat = (x - mu) * rstd (the forward's first product), a = dy * g: one rounding each.
//   5. c1 = wave_sum(sum of a) / H and c2 = wave_sum(sum of a * xhat) / H: the lane's elements in index order, then the butterfly; every
//      term passes through at most H / 64 + 6 additions.
//   6. dx = rstd * ((a - c1) - xhat * c2), rounded to fp16 once for dx16 and not at all for dx32.
//   7. dg += dy * xhat and db += dy per row in the wave's row order; ((w0 + w1) + w2) + w3 over the waves; the chunks strand by strand, the
//      strands in order; the old value last. At most rows_per_chunk / 4 + 4 + S + 1 additions per element. dg and db are not rounded again.
// Non-finite values propagate by IEEE rules alone: nothing is clamped, compared or used as an index.
#include <algorithm>
#include <type_traits>

#include "mdr_grad_common.h"
#include "../../include/mdr_layernorm_grad.h"

namespace mdr {
namespace {

typedef _Float16 lg_half4 __attribute__((ext_vector_type(4)));
typedef float lg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kLgWaves = 4;
constexpr int kLgThreads = 64 * kLgWaves;
constexpr int kLgMaxH = kGradMaxH;
constexpr int kLgPerLane = kLgMaxH / 64;
constexpr int kLgPlanes = 2;  // dg, db: the partial sums are [S][2][H]

// the lane's element k = i * W + j  <->  column (VEC ? (lane + 64 i) * 4 + j : lane + 64 i), W = VEC ? 4 : 1
template <typename T, bool VEC>
__device__ __forceinline__ void lg_load(const T* __restrict__ row, int lane, int i, float* out) {
    if constexpr (VEC) {
        if constexpr (std::is_same<T, float>::value) {
            const lg_f32x4 v = *(const lg_f32x4*)(row + (lane + 64 * i) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = v[j];
        } else {
            const lg_half4 v = *(const lg_half4*)(row + (lane + 64 * i) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = (float)v[j];
        }
    } else {
        out[0] = (float)row[lane + 64 * i];
    }
}

template <typename IN_T, int NV>
__global__ void __launch_bounds__(kLgThreads)
ln_grad_kernel(const IN_T* __restrict__ in, const _Float16* __restrict__ res16, const float* __restrict__ res32, const _Float16* __restrict__ dy16,
               const void* __restrict__ dy2, int dy2_f32, int M, const int* __restrict__ m_dev, int H, int rpc, const float* __restrict__ g, float eps,
               _Float16* __restrict__ dx16, float* __restrict__ dx32, float* dg, float* db, int accumulate, float* __restrict__ part) {
    constexpr bool VEC = NV > 0;
    constexpr int W = VEC ? 4 : 1;               // columns per group
    constexpr int NG = VEC ? NV : kLgPerLane;    // groups per lane (generic path: at most; n says how many)
    constexpr int NE = NG * W;                   // elements per lane
    __shared__ float red[kLgWaves][2][kLgMaxH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = VEC ? NV : H >> 6;             // groups per lane
    int rows = M;
    if (m_dev) rows = min(max(*m_dev, 0), M);
    const int r0 = blockIdx.x * rpc, r1 = min(r0 + rpc, rows);

    float gv[NE], dgv[NE], dbv[NE];
#pragma unroll
    for (int i = 0; i < NG; ++i) {
        if (i < n) lg_load<float, VEC>(g, lane, i, gv + i * W);
#pragma unroll
        for (int j = 0; j < W; ++j) dgv[i * W + j] = dbv[i * W + j] = 0.f;
    }

    for (int t = r0 + wave; t < r1; t += kLgWaves) {
        const size_t off = (size_t)t * H;
        float x[NE], dy[NE];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NG; ++i)
            if (i < n) {
                float* xi = x + i * W;
                float* di = dy + i * W;
                float tmp[W];
                lg_load<IN_T, VEC>(in + off, lane, i, xi);
                if (res16) {
                    lg_load<_Float16, VEC>(res16 + off, lane, i, tmp);
#pragma unroll
                    for (int j = 0; j < W; ++j) xi[j] += tmp[j];
                }
                if (res32) {
                    lg_load<float, VEC>(res32 + off, lane, i, tmp);
#pragma unroll
                    for (int j = 0; j < W; ++j) xi[j] += tmp[j];
                }
                if constexpr (VEC) s += xi[0] + xi[1] + xi[2] + xi[3];
                else s += xi[0];
                if (dy16) {
                    lg_load<_Float16, VEC>(dy16 + off, lane, i, di);
                    if (dy2) {
                        if (dy2_f32) lg_load<float, VEC>((const float*)dy2 + off, lane, i, tmp);
                        else lg_load<_Float16, VEC>((const _Float16*)dy2 + off, lane, i, tmp);
#pragma unroll
                        for (int j = 0; j < W; ++j) di[j] += tmp[j];
                    }
                } else {
                    if (dy2_f32) lg_load<float, VEC>((const float*)dy2 + off, lane, i, di);
                    else lg_load<_Float16, VEC>((const _Float16*)dy2 + off, lane, i, di);
                }
            }
        const float mu = grad_wave_sum(s) / H;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < NE; ++k)
            if (k < n * W) { const float dlt = x[k] - mu; v += dlt * dlt; }
        const float rstd = rsqrtf(grad_wave_sum(v) / H + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NE; ++k)
            if (k < n * W) {
                const float xh = (x[k] - mu) * rstd;
                const float a = dy[k] * gv[k];
                s1 += a;
                s2 += a * xh;
                dgv[k] += dy[k] * xh;
                dbv[k] += dy[k];
                x[k] = xh;
                dy[k] = a;
            }
        const float c1 = grad_wave_sum(s1) / H, c2 = grad_wave_sum(s2) / H;
#pragma unroll
        for (int i = 0; i < NG; ++i)
            if (i < n) {
                float d[W];
#pragma unroll
                for (int j = 0; j < W; ++j) d[j] = rstd * ((dy[i * W + j] - c1) - x[i * W + j] * c2);
                if constexpr (VEC) {
                    const size_t e = off + (lane + 64 * i) * 4;
                    if (dx16) *(lg_half4*)(dx16 + e) = (lg_half4){(_Float16)d[0], (_Float16)d[1], (_Float16)d[2], (_Float16)d[3]};
                    if (dx32) *(lg_f32x4*)(dx32 + e) = (lg_f32x4){d[0], d[1], d[2], d[3]};
                } else {
                    const size_t e = off + lane + 64 * i;
                    if (dx16) dx16[e] = (_Float16)d[0];
                    if (dx32) dx32[e] = d[0];
                }
            }
    }
    if (!dg && !db) return;  // (uniform over the workgroup)

#pragma unroll
    for (int i = 0; i < NG; ++i)
        if (i < n) {
            if constexpr (VEC) {
                const int e = (lane + 64 * i) * 4;
                *(lg_f32x4*)&red[wave][0][e] = (lg_f32x4){dgv[i * 4], dgv[i * 4 + 1], dgv[i * 4 + 2], dgv[i * 4 + 3]};
                *(lg_f32x4*)&red[wave][1][e] = (lg_f32x4){dbv[i * 4], dbv[i * 4 + 1], dbv[i * 4 + 2], dbv[i * 4 + 3]};
            } else {
                red[wave][0][lane + 64 * i] = dgv[i];
                red[wave][1][lane + 64 * i] = dbv[i];
            }
        }
    __syncthreads();
    for (int e = tid; e < H; e += kLgThreads) {
        const float sg = ((red[0][0][e] + red[1][0][e]) + red[2][0][e]) + red[3][0][e];
        const float sb = ((red[0][1][e] + red[1][1][e]) + red[2][1][e]) + red[3][1][e];
        if (part) {
            part[((size_t)blockIdx.x * 2) * H + e] = sg;
            part[((size_t)blockIdx.x * 2 + 1) * H + e] = sb;
        } else {
            if (dg) dg[e] = accumulate ? sg + dg[e] : sg;
            if (db) db[e] = accumulate ? sb + db[e] : sb;
        }
    }
}

// part [S][NP][H] -> the NP outputs. A workgroup owns 64 columns of one plane, a wave is a strand: strand j adds chunks j, j + 16, ... in
// order, then the first wave adds the min(S, 16) strands in order, then the old value.
__global__ void __launch_bounds__(64 * kGradStrands)
grad_strand_reduce_kernel(const float* __restrict__ part, int S, int NP, int H, float* o0, float* o1, float* o2, int accumulate) {
    __shared__ float st[kGradStrands][64];
    const int col = threadIdx.x & 63, strand = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + col;  // < NP H: the grid is NP H / 64 workgroups
    const int pl = (i >= H) + (i >= 2 * H), e = i - pl * H;  // i / H for NP <= 3 without the division (uniform over the workgroup: H is a multiple of 64)
    float* out = pl == 0 ? o0 : (pl == 1 ? o1 : o2);
    if (!out) return;
    const size_t chunk = (size_t)NP * H;  // floats of one chunk's partial sums
    const float* p = part + strand * chunk + (size_t)pl * H + e;
    float acc = 0.f;
#pragma unroll 8
    for (int c = strand; c < S; c += kGradStrands, p += kGradStrands * chunk) acc += *p;
    st[strand][col] = acc;
    __syncthreads();
    if (strand != 0) return;
    const int ns = min(S, kGradStrands);
    for (int j = 1; j < ns; ++j) acc += st[j][col];
    out[e] = accumulate ? acc + out[e] : acc;
}

__global__ void __launch_bounds__(256) gather_cls_grad_kernel(const _Float16* __restrict__ d, const int* __restrict__ cu, int B, int H, _Float16* __restrict__ acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, e = i - b * H;
    const int start = cu[b];
    if (cu[b + 1] <= start) return;  // an empty sequence owns no row
    _Float16* o = acc + (size_t)start * H + e;
    *o = (_Float16)((float)*o + (float)d[i]);
}

template <typename IN_T>
void lg_launch(int H, dim3 grid, hipStream_t st, const IN_T* in, const _Float16* res16, const float* res32, const _Float16* dy16, const void* dy2,
               int dy2_f32, int M, const int* m_dev, int rpc, const float* g, float eps, _Float16* dx16, float* dx32, float* dg, float* db, int accumulate,
               float* part) {
#define MDR_LG_LAUNCH(NV)                                                                                                                        \
    hipLaunchKernelGGL((ln_grad_kernel<IN_T, NV>), grid, dim3(kLgThreads), 0, st, in, res16, res32, dy16, dy2, dy2_f32, M, m_dev, H, rpc, g, eps, dx16, \
                       dx32, dg, db, accumulate, part)
    switch ((H & 255) == 0 ? H >> 8 : 0) {
        case 1: MDR_LG_LAUNCH(1); break;
        case 2: MDR_LG_LAUNCH(2); break;
        case 3: MDR_LG_LAUNCH(3); break;
        case 4: MDR_LG_LAUNCH(4); break;
        default: MDR_LG_LAUNCH(0); break;
    }
#undef MDR_LG_LAUNCH
}

}  // namespace

int launch_strand_reduce(const float* part, int S, int planes, int H, float* o0, float* o1, float* o2, int accumulate, hipStream_t stream) {
    hipLaunchKernelGGL(grad_strand_reduce_kernel, dim3(planes * H / 64), dim3(64 * kGradStrands), 0, stream, part, S, planes, H, o0, o1, o2, accumulate);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // namespace mdr

extern "C" {

int mdr_layernorm_backward_chunks(int M, int H, int* rows_per_chunk) {
    using namespace mdr;
    int rpc = 0, S = 0;
    if (M >= 1 && grad_hidden_ok(H)) S = grad_row_chunks(M, H, kLgPlanes, &rpc);
    if (rows_per_chunk) *rows_per_chunk = rpc;
    return S;
}

size_t mdr_layernorm_backward_workspace_bytes(int M, int H, int want) {
    using namespace mdr;
    if (!(M >= 1 && grad_hidden_ok(H))) return 0;
    int rpc;
    const int S = grad_row_chunks(M, H, kLgPlanes, &rpc);
    if (S == 1 || !(want & (MDR_LAYERNORM_WANT_DG | MDR_LAYERNORM_WANT_DB))) return 0;
    return align_up((size_t)S * 2 * H * sizeof(float), 256);
}

int mdr_layernorm_backward(const void* in_dev, int in_f16, const void* res16_dev, const float* res32_dev, const void* dy16_dev, const void* dy2_dev,
                           int dy2_f32, int M, const int* m_dev, int H, const float* g_dev, float eps, void* dx16_dev, float* dx32_dev, float* dg_dev,
                           float* db_dev, int accumulate, void* workspace_dev, size_t workspace_bytes, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_layernorm_backward";
    MDR_REQUIRE(in_dev && g_dev, "%s: NULL pointer (in and g are required)", fn);
    MDR_REQUIRE(dy16_dev || dy2_dev, "%s: NULL pointer (dy16 and dy2: at least one is required)", fn);
    MDR_REQUIRE(!(res16_dev && res32_dev), "%s: at most one of res16 / res32", fn);
    MDR_REQUIRE(dx16_dev || dx32_dev || dg_dev || db_dev, "%s: NULL pointer (every output: at least one is required)", fn);
    MDR_REQUIRE(in_f16 == 0 || in_f16 == 1, "%s: in_f16 must be 0 or 1, got %d", fn, in_f16);
    MDR_REQUIRE(dy2_f32 == 0 || dy2_f32 == 1, "%s: dy2_f32 must be 0 or 1, got %d", fn, dy2_f32);
    MDR_REQUIRE(M >= 1, "%s: M=%d must be at least 1", fn, M);
    MDR_REQUIRE(grad_hidden_ok(H), "%s: H=%d unsupported (a multiple of 64, 64 .. 1024)", fn, H);
    MDR_REQUIRE(aligned16({in_dev, res16_dev, res32_dev, dy16_dev, dy2_dev, g_dev, dx16_dev, dx32_dev, dg_dev, db_dev, workspace_dev}),
                "%s: every pointer must be 16-byte aligned", fn);
    int rpc;
    const int S = grad_row_chunks(M, H, kLgPlanes, &rpc);
    const bool sums = dg_dev || db_dev;
    const size_t need = S > 1 && sums ? (size_t)S * 2 * H * sizeof(float) : 0;
    MDR_REQUIRE_WORKSPACE(fn, workspace_dev, workspace_bytes, need, "mdr_layernorm_backward_workspace_bytes");
    MDR_ENTER_DEVICE(device);
    hipStream_t st = (hipStream_t)stream;
    float* part = need ? (float*)workspace_dev : nullptr;
    if (in_f16)
        lg_launch(H, dim3(S), st, (const _Float16*)in_dev, (const _Float16*)res16_dev, res32_dev, (const _Float16*)dy16_dev, dy2_dev, dy2_f32, M, m_dev, rpc,
                  g_dev, eps, (_Float16*)dx16_dev, dx32_dev, dg_dev, db_dev, accumulate ? 1 : 0, part);
    else
        lg_launch(H, dim3(S), st, (const float*)in_dev, (const _Float16*)res16_dev, res32_dev, (const _Float16*)dy16_dev, dy2_dev, dy2_f32, M, m_dev, rpc,
                  g_dev, eps, (_Float16*)dx16_dev, dx32_dev, dg_dev, db_dev, accumulate ? 1 : 0, part);
    MDR_HIP_TRY(hipGetLastError());
    if (part) return launch_strand_reduce(part, S, kLgPlanes, H, dg_dev, db_dev, nullptr, accumulate ? 1 : 0, st);
    return MDR_OK;
}

int mdr_gather_cls_backward(const void* d16_dev, const int* cu_dev, int B, int H, void* acc16_dev, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_gather_cls_backward";
    MDR_REQUIRE(d16_dev && cu_dev && acc16_dev, "%s: NULL pointer (d16, cu and acc16 are required)", fn);
    MDR_REQUIRE(B >= 1 && B <= (1 << 20), "%s: B=%d out of range (1 .. 2^20)", fn, B);
    MDR_REQUIRE(grad_hidden_ok(H), "%s: H=%d unsupported (a multiple of 64, 64 .. 1024)", fn, H);
    MDR_REQUIRE(aligned16({d16_dev, acc16_dev}), "%s: d16 and acc16 must be 16-byte aligned", fn);
    MDR_ENTER_DEVICE(device);
    hipLaunchKernelGGL(gather_cls_grad_kernel, dim3((B * H + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const _Float16*)d16_dev, cu_dev, B, H,
                       (_Float16*)acc16_dev);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // extern "C"
