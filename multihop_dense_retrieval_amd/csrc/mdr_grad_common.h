// csrc/mdr_grad_common.h -- what the stand-alone gradient translation units share (mdr_attention_grad.hip, mdr_layernorm_grad.hip,
// mdr_embedding_grad.hip; NOT mdr_encoder.hip, whose own wave_sum lives in that unit's anonymous namespace): the wave reduction, the limits
// of H, the split of the rows into chunks, and the launcher of the strand reduce that turns the chunks' partial sums into the outputs.
#pragma once
#include <algorithm>

#include "mdr_common.h"

namespace mdr {

constexpr int kGradMaxH = 1024;
constexpr int kGradStrands = 16;                          // chains of grad_strand_reduce_kernel over the chunks
constexpr int kGradMaxChunks = 1024;                      // target number of workgroups ...
constexpr size_t kGradMaxPartialBytes = (size_t)4 << 20;  // ... as far as the partial sums [S][planes][H] stay within 4 MiB

// the xor butterfly 32, 16, .. 1 (wave_sum of csrc/mdr_encoder_pack_ln.inl)
__device__ __forceinline__ float grad_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

inline bool grad_hidden_ok(int H) { return H >= 64 && H <= kGradMaxH && H % 64 == 0; }

// (S, rows per chunk) of M rows whose chunks each leave `planes` rows of H partial sums: a function of (M, H, planes) alone
inline int grad_row_chunks(int M, int H, int planes, int* rpc_out) {
    const int most = (int)std::min<size_t>(kGradMaxChunks, kGradMaxPartialBytes / (planes * sizeof(float) * (size_t)H));
    const int rpc = ((M + most - 1) / most + 3) / 4 * 4;
    *rpc_out = rpc;
    return (M + rpc - 1) / rpc;
}

// part [S][planes][H] -> the `planes` outputs o0, o1, o2 (NULL: that plane is skipped) of H floats each: grad_strand_reduce_kernel of
// csrc/mdr_layernorm_grad.hip on planes * H / 64 workgroups of 64 * 16 threads. Strand j of sixteen adds chunks j, j + 16, ... in order,
// the min(S, 16) strands are added in strand order, then (accumulate) the old value.
int launch_strand_reduce(const float* part, int S, int planes, int H, float* o0, float* o1, float* o2, int accumulate, hipStream_t stream);

}  // namespace mdr
