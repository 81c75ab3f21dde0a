// csrc/mdr_gemm_choice.h -- which of the forward GEMM kernels a call runs on: the ONE statement of launch_gemm's decision (csrc/mdr_encoder.hip).
// Host integers in, a kernel id out; nothing here launches, reads the environment or touches a device. launch_gemm switches on the answer and the
// mdr_test_gemm_choice hook (include/mdr_hip.h) reports it, so the tests read the choice the launcher makes instead of restating it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

namespace mdr {

constexpr int kPersistBiasMax = 3072;  // floats of bias kept in LDS behind the ring (12 KiB)

// ---- tail of the persistent 256x256 kernels: the last, partial round on 128x128 tiles ------------------------------------------
// T = ntm x ntn tiles of 256x256 over G persistent workgroups take ceil(T / G) rounds; when T is a little over a multiple of G the last round
// keeps a few workgroups busy for a whole tile time while the rest of the chip idles (86 row tiles of 256 x N = 768: 258 tiles = TWO rounds on 256
// CUs for one round of work -- the +37 % step at 21.8 k tokens of DESIGN.md section 4). gemm_head_row_tiles() gives the 256x256 walk only the row
// tiles that fill COMPLETE rounds; the remaining rows (fewer than max_rem + ntn tiles' worth) are computed by the same workgroups afterwards on
// 128x128 tiles (gemm_tail_tile: the one-tile-per-block kernel's K-loop on a four-slot ring over the whole 128 KiB), which spreads them over 4x as many units. Same K order and MFMA per output element as every other flavour: bit-identical results.
__host__ __device__ inline int gemm_head_row_tiles(int ntm, int ntn, int G, int max_rem) {
    const long long T = (long long)ntm * ntn;
    const long long full = T / G, rem = T % G;
    if (full < 1 || rem == 0 || rem > max_rem) return ntm;
    return (int)(full * G / ntn);
}

// Rounds of tiles the busiest workgroup walks (tiles split evenly over 8 XCDs, then round-robin over an XCD's workgroups).
inline int persistent_rounds(int M_est, int bm, int N, int bn, int wgs_per_xcd) {
    const long long T = (long long)((M_est + bm - 1) / bm) * (N / bn);
    const long long per_xcd = (T + 7) / 8;
    return (int)((per_xcd + wgs_per_xcd - 1) / wgs_per_xcd);
}

// kernel: 1 = 64x64, 2 = 128x128, 3 = the one-tile 256-wide GemmBig (MDR_GEMM_CFG=3 only), 4 = persistent 256x128, 6 / 7 = persistent 256x256 on eight /
// four waves, 8-13 = the measurement tile shapes of MDR_GEMM_EXTRA_CFGS builds. res_added: the kernel adds the residual of EPI_BIAS_RES_F32 itself (the
// one-tile kernels); the persistent ones leave it to the LayerNorm that follows.
struct GemmChoice {
    int kernel;
    bool res_added;
};

// sel: 0 = the heuristic, else the selection of MDR_GEMM_CFG (1 small, 2 mid, 3 big tiles; 4 persistent 256x128 / 6, 7 persistent 256x256 for the large-M
// calls, the others keep the heuristic) or, forced, of a test hook's `kernel` (which holds at any M_est). A selection whose condition the shape does not
// meet falls back: 7 and 6 to 4, 4 and 2 to 1. M_est: expected number of valid rows (the packed token count is only known on the device). out_bytes: 4 for
// the fp32 epilogues (EPI_BIAS_RES_F32 runs as EPI_BIAS_F32 on a persistent kernel), 2 for the fp16 ones.
inline GemmChoice gemm_choose(int sel, bool forced, int M_cap, int M_est, int N, int K, int lda, int ldo, int out_bytes, int num_cus) {
    const long long p_tiles = (long long)(N / 128) * ((M_est + 255) / 256);
    if (!forced && (sel == 4 || sel == 6 || sel == 7) && p_tiles < (long long)num_cus * 3 / 2) sel = 0;
    if ((sel == 4 || sel == 6 || sel == 7 || (sel == 0 && p_tiles >= (long long)num_cus * 3 / 2)) && N % 128 == 0 && N <= kPersistBiasMax) {
        // Both kernels are bound by the bytes a CU moves over its L2 path, loads AND stores (~20 B/clk/CU measured; skipping
        // the stores made the K = 768 GEMMs 25-30 % faster, deferring them did not): cost = rounds x (tile inputs + outputs).
        // the 256x256 kernels store through a buffer descriptor with 32-bit byte offsets: outputs of 4 GiB and more go to the 256x128 kernel
        // (the offsets of the LAST row tile reach row M + 254: the guard covers M_cap + 255 rows, so that they cannot wrap into valid low rows -- ADVICE r3)
        const bool out32 = ((unsigned long long)M_cap + 255ull) * (unsigned long long)ldo * (out_bytes == 4 ? 4ull : 2ull) < (1ull << 32);
        const bool a32 = ((unsigned long long)M_cap + 255ull) * (unsigned long long)lda * 2ull < (1ull << 32);  // the four-wave kernel also LOADS A through a descriptor
        if (sel == 7 && out32 && a32 && N % 256 == 0 && K % 128 == 0 && K >= 256) return {7, false};
        if ((sel == 6 || sel == 0) && N % 256 == 0 && out32) {
            const double osz = (out_bytes == 4) ? 4.0 : 2.0;
            // the 256x256 kernels walk only the row tiles that fill complete rounds and finish the rest on 128x128 tiles (gemm_head_row_tiles): cost =
            // complete rounds x big tile + passes x small tile (latency-bound: counted 1.5 x its bytes)
            const int grid = num_cus / 8 * 8, ntm_all = (M_est + 255) / 256;
            auto cost256 = [&](int max_rem, int tiles_per_pass, int* rounds_out) {
                const int head = gemm_head_row_tiles(ntm_all, N / 256, grid, max_rem);
                const int rounds = persistent_rounds(std::min(M_est, head * 256), 256, N, 256, num_cus / 8);
                const long long tail_tiles = (long long)((std::max(0, M_est - head * 256) + 127) / 128) * (N / 128);
                const long long passes = (tail_tiles + (long long)grid * tiles_per_pass - 1) / ((long long)grid * tiles_per_pass);
                if (rounds_out) *rounds_out = rounds;
                return rounds * ((256.0 + 256.0) * K * 2 + 256.0 * 256.0 * osz) + passes * 1.2 * ((128.0 + 128.0) * K * 2 + 128.0 * 128.0 * osz);
            };
            int rounds_q = 0;
            const double c_quad = cost256(grid / 4, 1, &rounds_q), c_big = cost256(grid / 2, 1, nullptr);
            const double c_p = persistent_rounds(M_est, 256, N, 128, num_cus / 8) * ((256.0 + 128.0) * K * 2 + 256.0 * 128.0 * osz);
            if (sel == 6 || std::min(c_big, c_quad) < c_p) {
                // four waves of 128x128 (gemm_quad_kernel): a faster K-loop (fewer LDS reads, one barrier per K-tile) behind a slower epilogue (one
                // wave per SIMD has nobody to hide its latencies). Measured at 20.3 k rows: FFN2 77 vs 83-86 us, out-projection 30-33 vs 31-37,
                // but QKV 84-89 vs 70-72 and FFN1 113-123 vs 106-117 (three / four tiles per workgroup, K = 768): taken where the K-loop dominates.
                if (sel == 0 && a32 && K % 128 == 0 && K >= 256 && (rounds_q == 1 || K >= 2048) && c_quad <= 1.15 * c_big) return {7, false};
                return {6, false};
            }
        }
        return {4, false};
    }
    const long long big_blocks = (N % 256 == 0) ? (long long)(N / 256) * ((M_est + 255) / 256) : 0;
    const long long mid_blocks = (long long)(N / 128) * ((M_est + 127) / 128);
    const long long small_blocks = (long long)(N / 64) * ((M_est + 63) / 64);
    if (sel == 3 && big_blocks > 0) return {3, true};
#ifdef MDR_GEMM_EXTRA_CFGS  // measurement builds: more tile shapes behind the test hook's kernel ids 8-13
    if (sel >= 8 && sel <= 13) return {sel, true};
#endif
    // bytes the busiest CU pulls through its L2 path: rounds of blocks x (BM + BN) rows of K; ties go to the small tile
    // (measured at 2.4 k rows: QKV / FFN1 faster on 128x128, out-projection / FFN2 on 64x64)
    const long long c_mid = (mid_blocks + num_cus - 1) / num_cus * 256, c_small = (small_blocks + num_cus - 1) / num_cus * 128;
    // (a forced 128x128 selection whose N is no multiple of 128 takes the 64x64 kernel, as the forced persistent selections do: the grid of the
    // 128x128 kernel would leave the last 64 columns unwritten)
    if (N % 128 == 0 && (sel == 2 || (sel == 0 && c_mid < c_small))) return {2, true};
    return {1, true};
}

}  // namespace mdr
