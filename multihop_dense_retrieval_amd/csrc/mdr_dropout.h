// csrc/mdr_dropout.h -- the dropout mask of the training bricks (include/mdr_dropout.h), written once: Philox4x32-10 (Salmon, Moraes, Dror,
// Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011) and the two mappings from an element to a byte of one generator call.
// Device header of csrc/mdr_dropout.hip (row kernel, test hook) and csrc/mdr_attention_grad.hip (training forward, backward with dropout);
// tests/dropout_ref.py is its numpy replica.
//
// The mask is a PURE FUNCTION of (seed: uint64, site: uint32, the element's indices, T): it does not depend on L, the launch geometry, which
// pass asks, or the rest of the batch. The forward draws it, the backward replays it; nothing is stored.
//   key      = (seed & 0xffffffff, seed >> 32)
//   bytes    one call yields four words = 16 bytes; byte k = (word[k >> 2] >> (8 (k & 3))) & 0xff
//   keep     an element is kept iff its byte >= T, T = floor(256 p + 0.5) in 0 .. 255. T = 0 keeps everything.
//   rate     the rate actually drawn is p_eff = T / 256, NOT the nominal p: p = 0.1 draws 26 / 256 = 0.1016. Eight bits per element is one
//            generator call per 16 hidden elements or per 4 x 4 block of probabilities. The scale is fp32(256 / (256 - T)), so the expectation
//            is exact for p_eff.
//   factor   the mask value is m in {0, scale} and is applied as an IEEE MULTIPLICATION, never a select: a non-finite value at a dropped
//            position becomes NaN (as torch's x * mask makes it), so the overflow contract stays conservative.
//   hidden   element (row, col) of an [M, N] tensor, N % 16 == 0: byte col & 15 of counter (col >> 4, row, 0, site).
//   attention  probability of query i, key j (both sequence-local), head h, sequence b (the index in the call's cu): byte 4 (i & 3) + (j & 3)
//            of counter (i >> 2, j >> 2, b * heads + h, site). The first-query mode is the same function at i = 0. The mask DOES depend on b:
//            with dropout a sequence's output and gradient depend on its place in the batch, as torch's do.
//   unique   it is the CALLER's duty to give every use its own site or seed: every step, encode, layer and place. Two uses that share
//            (seed, site) share their mask.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace mdr {

struct DropoutParams {  // by value into the kernels
    uint32_t k0, k1;    // the Philox key
    uint32_t site;
    uint32_t T;         // threshold 0 .. 255
    float scale;        // fp32(256 / (256 - T))
};

inline DropoutParams dropout_params(unsigned T, uint64_t seed, uint32_t site) {
    return DropoutParams{(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), site, T, (float)(256.0 / (256.0 - (double)T))};
}

// T of a rate p, -1 for a p outside [0, 1) or one that rounds to 256
inline int dropout_threshold(float p) {
    if (!(p >= 0.f && p < 1.f)) return -1;
    const int T = (int)((double)p * 256.0 + 0.5);
    return T >= 256 ? -1 : T;
}

__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return uint4{c0, c1, c2, c3};
}

// m of byte k (0 .. 3) of one word
__device__ __forceinline__ float dropout_factor(uint32_t word, int k, const DropoutParams& dp) {
    return ((word >> (8 * k)) & 0xffu) >= dp.T ? dp.scale : 0.f;
}

// The attention site. A lane of attn_grad_kernel holds four consecutive swept rows of one owner: one call serves them.
// Row pass (owner = query i, swept = keys 4 jb .. 4 jb + 3): the four bytes of word i & 3.
__device__ __forceinline__ uint32_t dropout_attn_word_keys(int i, int jb, uint32_t bh, const DropoutParams& dp) {
    const uint4 w = philox4x32_10((uint32_t)i >> 2, (uint32_t)jb, bh, dp.site, dp.k0, dp.k1);
    const int r = i & 3;
    return r == 0 ? w.x : r == 1 ? w.y : r == 2 ? w.z : w.w;
}

// Column pass (owner = key j, swept = queries 4 ib .. 4 ib + 3): byte j & 3 of each word, gathered into one word (byte r <-> query 4 ib + r).
__device__ __forceinline__ uint32_t dropout_attn_word_queries(int ib, int j, uint32_t bh, const DropoutParams& dp) {
    const uint4 w = philox4x32_10((uint32_t)ib, (uint32_t)j >> 2, bh, dp.site, dp.k0, dp.k1);
    const int sh = 8 * (j & 3);
    return ((w.x >> sh) & 0xffu) | (((w.y >> sh) & 0xffu) << 8) | (((w.z >> sh) & 0xffu) << 16) | (((w.w >> sh) & 0xffu) << 24);
}

}  // namespace mdr
