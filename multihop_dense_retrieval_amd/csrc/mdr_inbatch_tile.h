// csrc/mdr_inbatch_tile.h -- device helpers shared by the in-batch rank step (mdr_inbatch.hip) and the in-batch loss and its
// gradients (mdr_inbatch_grad.hip): the staged-query tile types, the 16 x 32 score tile on MFMA and the online log-sum-exp.
// Both translation units call the same code, so a score or a log-sum-exp has the same bits in either.
#pragma once
#include <cfloat>
#include <cmath>

#include "mdr_common.h"

#include "../../include/mdr_inbatch.h"

namespace mdr {
namespace {

typedef _Float16 ib_half8 __attribute__((ext_vector_type(8)));
typedef float ib_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kIbQT = 32;  // query rows per workgroup: two 16-row MFMA subtiles
constexpr int kIbWaves = 8;
constexpr int kIbThreads = kIbWaves * 64;
constexpr int kIbMaxD = 1024;

template <int MODE>
struct IbElem {  // MDR_INBATCH_F32: the query tile stays fp32; rows padded by 16 bytes against LDS bank conflicts
    using T = float;
    static constexpr int PAD = 4;
};
template <>
struct IbElem<MDR_INBATCH_O1> {
    using T = _Float16;
    static constexpr int PAD = 8;
};

template <int MODE>
__device__ __forceinline__ float ib_score(float acc) {
    return MODE == MDR_INBATCH_O1 ? (float)(_Float16)acc : acc;  // O1: torch.mm returns fp16 (round to nearest even)
}

// One 16 (context rows) x 32 (queries) tile over all of K. `a` = this lane's context row, `qt` = the staged query tile.
// Operand maps (lane l, c = l & 15, g = l >> 4): 16x16x4 f32 takes A[row c][k slot g], 16x16x32 f16 takes A[row c][k = 8g .. 8g + 7]
// and the same for B[.][col c]; C[row 4g + r][col c] is in register r. For fp32 a lane loads 4 consecutive k and feeds
// them to 4 MFMAs, i.e. MFMA e of a 16-wide step sums k = 4g + e over g: a permutation of K that A and B share.
template <int MODE>
__device__ __forceinline__ void tile_mma(const float* __restrict__ a, const typename IbElem<MODE>::T* qt, int stride, int d, int lane,
                                         ib_f32x4& acc0, ib_f32x4& acc1) {
    const int c = lane & 15, g = lane >> 4;
    acc0 = ib_f32x4{0.f, 0.f, 0.f, 0.f};
    acc1 = ib_f32x4{0.f, 0.f, 0.f, 0.f};
    if (MODE == MDR_INBATCH_F32) {
        const float* ap = a + 4 * g;
        const float* b0 = (const float*)qt + c * stride + 4 * g;
        const float* b1 = b0 + 16 * stride;
        float4 x = *(const float4*)ap;
        for (int k = 0; k < d; k += 16) {
            float4 nx = x;
            if (k + 16 < d) nx = *(const float4*)(ap + k + 16);  // the next step's context operand, ahead of this step's MFMAs
            const float4 y0 = *(const float4*)(b0 + k);
            const float4 y1 = *(const float4*)(b1 + k);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, y0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, y1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, y0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, y1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, y0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, y1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, y0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, y1.w, acc1, 0, 0, 0);
            x = nx;
        }
    } else {
        const float* ap = a + 8 * g;
        const _Float16* b0 = (const _Float16*)qt + c * stride + 8 * g;
        const _Float16* b1 = b0 + 16 * stride;
        float4 x0 = *(const float4*)ap, x1 = *(const float4*)(ap + 4);
        for (int k = 0; k < d; k += 32) {
            float4 n0 = x0, n1 = x1;
            if (k + 32 < d) {
                n0 = *(const float4*)(ap + k + 32);
                n1 = *(const float4*)(ap + k + 36);
            }
            const ib_half8 xh = {(_Float16)x0.x, (_Float16)x0.y, (_Float16)x0.z, (_Float16)x0.w,
                                 (_Float16)x1.x, (_Float16)x1.y, (_Float16)x1.z, (_Float16)x1.w};
            const ib_half8 y0 = *(const ib_half8*)(b0 + k);
            const ib_half8 y1 = *(const ib_half8*)(b1 + k);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, y0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, y1, acc1, 0, 0, 0);
            x0 = n0;
            x1 = n1;
        }
    }
}

// online log-sum-exp: (m, s) stands for m + log(s). A -inf term adds nothing, a NaN term makes s NaN, +inf terms count 1 each.
__device__ __forceinline__ void lse_fold(float& m, float& s, float x) {
    if (x == -INFINITY) return;
    if (x > m) {
        s = s * expf(m - x) + 1.f;
        m = x;
    } else {
        s += (x == m) ? 1.f : expf(x - m);
    }
}

__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    const float f1 = (m == M) ? 1.f : expf(m - M);
    const float f2 = (m2 == M) ? 1.f : expf(m2 - M);
    s = s * f1 + s2 * f2;
    m = M;
}

__device__ __forceinline__ float pick4(const ib_f32x4& v, int r) {
    return r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : v[3];
}

}  // namespace
}  // namespace mdr
