// csrc/mdr_encoder_dropout.inl -- the two row kernels of the encoder's training-mode forward (include/mdr_encoder_dropout.h): LayerNorm and
// embedding + LayerNorm with the hidden-state dropout of csrc/mdr_dropout.h folded in, so that a forward that keeps nothing for a backward
// makes no separate mask pass. Included by mdr_encoder.hip inside namespace mdr::{anonymous}, behind mdr_encoder_pack_ln.inl, whose
// kernels these are siblings of: same ownership of columns by lanes, same order of every sum, same expressions, so that with the mask
// applied in front (layernorm) or behind (embedding) the bits are those of the two-pass chain dropout_rows_kernel -> layernorm_kernel
// resp. embed_ln_kernel -> dropout_rows_kernel. The plain kernels are not touched.
//
// The mask of element (row, col) is byte col & 15 of the generator call with counter (col >> 4, row, 0, site).
//   fast path (H % 256 == 0): a lane owns the columns 4 (lane + 64 i) .. + 3, which are the four bytes of word lane & 3 of call
//     (lane + 64 i) >> 2: four neighbouring lanes want the four words of one call.
//   generic path: a lane owns the columns lane + 64 i, byte lane & 15 of call (lane >> 4) + 4 i: sixteen neighbouring lanes want one call.
// Every lane makes the call itself and keeps its word; nothing crosses lanes. The other choice is one call per group of lanes and a
// broadcast (a DPP quad permute, or ds_bpermute through the LDS crossbar). A call is ten rounds of two 32-bit multiplies, high and low
// halves (40 multiplies at a quarter of the VALU rate, about 8 cycles each for one wave on a 32-wide SIMD) and a dozen full-rate
// operations: at H = 768 a row costs a wave 3 calls, about a thousand SIMD cycles, against the 9 KiB the row moves (fp16 sums and fp32
// residual in, fp16 and fp32 out), which at the ~10 B/cycle a CU streams from HBM is about 900 cycles per row for the CU's four SIMDs
// together. The generator therefore stays at about a quarter of the memory time and overlaps with it at eight waves per SIMD; sharing
// would save three quarters of that quarter only if the kernel were VALU-bound, and costs a cross-lane dependency in front of the first
// add. The embedding (generic ownership, H / 64 calls per lane) runs once per encode against 2 * layers LayerNorms and is left alike.

__device__ __forceinline__ uint32_t pick_word(const uint4& w, int r) { return r == 0 ? w.x : r == 1 ? w.y : r == 2 ? w.z : w.w; }

// out16 / out32 = LayerNorm(fp32(fp16(fp32(in) * m)) + res32): layernorm_kernel<_Float16> with dropout_rows_kernel<true> in front, in
// registers. The inner rounding to fp16 is that kernel's one rounding point. m is a factor, not a select: a non-finite `in` at a dropped
// position is NaN. out32 may alias res32 (a wave reads its whole row before it writes it).
__global__ void __launch_bounds__(256)
layernorm_dropout_kernel(const _Float16* __restrict__ in, const float* res32, int rows_cap, const int* __restrict__ rows_dev, int H,
                         const float* __restrict__ g, const float* __restrict__ bta, float eps, DropoutParams dp, _Float16* __restrict__ out16,
                         float* out32) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int rows = rows_dev ? min(*rows_dev, rows_cap) : rows_cap;
    if (t >= rows) return;
    const _Float16* r = in + (size_t)t * H;
    if ((H & 255) == 0) {
        const int n4 = H >> 8;  // float4 per lane (<= 4)
        f32x4 x[4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n4) {
                const half4 h4 = *(const half4*)(r + (lane + 64 * i) * 4);
                const uint32_t word = pick_word(philox4x32_10((uint32_t)(lane + 64 * i) >> 2, (uint32_t)t, 0u, dp.site, dp.k0, dp.k1), lane & 3);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[i][j] = (float)(_Float16)((float)h4[j] * dropout_factor(word, j, dp));
                if (res32) x[i] += *(const f32x4*)(res32 + (size_t)t * H + (lane + 64 * i) * 4);
                s += x[i][0] + x[i][1] + x[i][2] + x[i][3];
            }
        const float mu = wave_sum(s) / H;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float dlt = x[i][j] - mu; v += dlt * dlt; }
            }
        const float rstd = rsqrtf(wave_sum(v) / H + eps);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n4) {
                const int e = (lane + 64 * i) * 4;
                const f32x4 g4 = *(const f32x4*)(g + e), b4 = *(const f32x4*)(bta + e);
                f32x4 y;
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = (x[i][j] - mu) * rstd * g4[j] + b4[j];
                if (out16) {
                    half4 o;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = (_Float16)y[j];
                    *(half4*)(out16 + (size_t)t * H + e) = o;
                }
                if (out32) *(f32x4*)(out32 + (size_t)t * H + e) = y;
            }
        return;
    }
    const int n = H >> 6;
    float x[kMaxPerLane];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxPerLane; ++i)
        if (i < n) {
            const uint32_t word = pick_word(philox4x32_10((uint32_t)(lane >> 4) + 4u * i, (uint32_t)t, 0u, dp.site, dp.k0, dp.k1), (lane >> 2) & 3);
            x[i] = (float)(_Float16)((float)r[lane + 64 * i] * dropout_factor(word, lane & 3, dp)) + 0.f + (res32 ? res32[(size_t)t * H + lane + 64 * i] : 0.f);
            s += x[i];
        }
    const float mu = wave_sum(s) / H;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxPerLane; ++i)
        if (i < n) { float dlt = x[i] - mu; v += dlt * dlt; }
    const float rstd = rsqrtf(wave_sum(v) / H + eps);
#pragma unroll
    for (int i = 0; i < kMaxPerLane; ++i)
        if (i < n) {
            int e = lane + 64 * i;
            float y = (x[i] - mu) * rstd * g[e] + bta[e];
            if (out16) out16[(size_t)t * H + e] = (_Float16)y;
            if (out32) out32[(size_t)t * H + e] = y;
        }
}

// embed_ln_kernel with dropout_rows_kernel<false> (y16 given) behind it, in registers: y32 = LN(word + pos + type) * m, one fp32 rounding,
// and y16 = fp16(y32), one rounding of the masked value. The row of the mask is the packed token.
__global__ void __launch_bounds__(256)
embed_ln_dropout_kernel(const long long* __restrict__ ids, const int* __restrict__ tok_src, const int* __restrict__ tok_pid, const int* __restrict__ total,
                        const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type0, const float* __restrict__ g,
                        const float* __restrict__ bta, int H, int vocab, int max_pos, float eps, DropoutParams dp, _Float16* __restrict__ out,
                        float* __restrict__ out32) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= *total) return;
    long long id = ids[tok_src[t]];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int pid = tok_pid[t];
    pid = pid >= max_pos ? max_pos - 1 : pid;
    const float* wr = word + (size_t)id * H;
    const float* pr = pos + (size_t)pid * H;
    const int n = H >> 6;
    float x[kMaxPerLane];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxPerLane; ++i)
        if (i < n) { int e = lane + 64 * i; x[i] = wr[e] + pr[e] + type0[e]; s += x[i]; }
    const float mu = wave_sum(s) / H;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxPerLane; ++i)
        if (i < n) { float dlt = x[i] - mu; v += dlt * dlt; }
    const float rstd = rsqrtf(wave_sum(v) / H + eps);
#pragma unroll
    for (int i = 0; i < kMaxPerLane; ++i)
        if (i < n) {
            const int e = lane + 64 * i;
            const float y = (x[i] - mu) * rstd * g[e] + bta[e];
            const uint32_t w = pick_word(philox4x32_10((uint32_t)(lane >> 4) + 4u * i, (uint32_t)t, 0u, dp.site, dp.k0, dp.k1), (lane >> 2) & 3);
            float yd = y * dropout_factor(w, lane & 3, dp);
            // y16 is fp16(fp32(y * m)), two roundings, as dropout_rows_kernel<false> stores it. Left alone hipcc folds the product into the
            // conversion (v_fma_mixlo_f16: one rounding of the exact product), an fp16 ulp away where the fp32 product sits near a tie: the
            // empty statement makes the rounded fp32 product the conversion's operand.
            asm volatile("" : "+v"(yd));
            out[(size_t)t * H + e] = (_Float16)yd;
            if (out32) out32[(size_t)t * H + e] = yd;
        }
}
