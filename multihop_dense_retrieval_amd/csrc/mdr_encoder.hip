// csrc/mdr_encoder.hip -- RoBERTa encoder forward + CLS projection for gfx950 (MI355X).
//
// Replaces   project(encoder(input_ids, mask)[0][:, 0, :])
//   /root/reference/mdr/retrieval/models/mhop_retriever.py:23-26,40-41   (RobertaRetriever.encode_q)
//   /root/reference/mdr/retrieval/models/retriever.py:186-190            (RobertaCtxEncoder.forward)
// where `encoder` is HuggingFace RobertaModel (transformers 2.11, third party). Numerics follow the
// apex-O1 regime the reference runs under (eval_mhop_retrieval.py:88-89): fp16 GEMM operands with fp32
// accumulation; LayerNorm, softmax and GELU in fp32. See DESIGN.md §4.
//
// Execution is UNPADDED: tokens whose mask is 0 are dropped up front (the CLS embedding does not
// depend on them) and every kernel works on the packed [T, hidden] token
// matrix; T is only known on the device, so grids are sized for batch*seq_len and surplus tiles exit.
//
// Kernels
//   enc_lens / enc_scan / enc_scatter   packing: lengths, cu_seqlens, token -> (row, position id)
//   embed_ln                            word + position + type embedding gather, LayerNorm -> fp16
//   gemm_f16<EPI,WM,STAGES>             C = A[M,K] x W[N,K]^T on v_mfma_f32_16x16x32_f16, (64..256)x128x64 tiles,
//                                       global_load_lds staging (XOR-swizzled via the source address),
//                                       fused bias / bias+GELU / bias+residual epilogues
//   attention<NT>                       per (sequence, head): K and V^T of the sequence staged in LDS once,
//                                       S = QK^T on MFMA, fp32 softmax in registers, O = PV on MFMA
//   layernorm                           fp32 [T,H] -> fp16 (hidden state) or fp32 (final embedding)
//   layernorm_dropout / embed_ln_dropout  the two above with the hidden-state dropout mask folded in (mdr_encoder_dropout.inl): the
//                                       training-mode forward of include/mdr_encoder_dropout.h
//
// Host side, in this order: the GEMM / attention launchers (here); the transformer trunk shared with the answer reader -- weights and their
// upload, workspace, packing prologue, layer body (mdr_encoder_trunk.inl); the encoder's own part -- its embedding launch, the CLS-only last
// layer, the projection head and the GEMM / attention test hooks (here); the reader (mdr_reader.inl, mdr_reader_assemble.inl); the test hooks of
// the packing / embedding / LayerNorm / row kernels (mdr_encoder_test_rows.inl).
#include <hip/hip_runtime.h>
#include <map>
#include <mutex>
#include <algorithm>
#include <type_traits>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mdr_common.h"
#include "mdr_dropout.h"
#include "mdr_gemm_choice.h"
#include "../../include/mdr_dropout.h"
#include "../../include/mdr_encoder_dropout.h"
#include "../../include/mdr_reader.h"

namespace mdr {
namespace {

#include "mdr_encoder_pack_ln.inl"
#include "mdr_encoder_dropout.inl"
#include "mdr_encoder_gemm.inl"
#include "mdr_encoder_gemm_quad.inl"
#include "mdr_encoder_attention.inl"

}  // namespace
}  // namespace mdr

// ======================================================================================================
// host side
// ======================================================================================================
using namespace mdr;

#ifndef MDR_CU_LANES
#define MDR_CU_LANES 0  // 1: measurement build with CU-partitioned lanes (include/mdr_hip_measure.h)
#endif

namespace {

template <int EPI, typename C>
int launch_gemm_cfg(const _Float16* A, int lda, const _Float16* W, const float* bias, int M_cap, const int* M_dev, int N, int K, void* out, int ldo,
                    const _Float16* res, int ldr, hipStream_t st) {
    { int rc_ = ensure_dynamic_lds((const void*)gemm_f16_kernel<EPI, C>, C::LDS_BYTES); if (rc_) return rc_; }
    const int blocks = (N / C::BN) * ((M_cap + C::BM - 1) / C::BM);
    hipLaunchKernelGGL((gemm_f16_kernel<EPI, C>), dim3(blocks), dim3(C::THREADS), C::LDS_BYTES, st, A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

template <int EPI, typename C>
int launch_gemm_persist(const _Float16* A, int lda, const _Float16* W, const float* bias, int M_cap, const int* M_dev, int N, int K, void* out, int ldo,
                        int num_cus, hipStream_t st) {
    constexpr int lds = C::LDS_BYTES + kPersistBiasMax * 4;
    { int rc_ = ensure_dynamic_lds((const void*)gemm_persist_kernel<EPI, C>, lds); if (rc_) return rc_; }
    const int grid = num_cus / 8 * 8;
    // MDR_GEMM_EPI (compile-time, measurement builds): 0 stores after the tile, 1 deferred, 2 (product) deferred + two stores may stay in flight
    hipLaunchKernelGGL((gemm_persist_kernel<EPI, C>), dim3(grid), dim3(C::THREADS), lds, st, A, lda, W, bias, M_cap, M_dev, N, K, out, ldo,
                       MDR_GEMM_EPI);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

template <int EPI>
int launch_gemm_big(const _Float16* A, int lda, const _Float16* W, const float* bias, int M_cap, const int* M_dev, int N, int K, void* out, int ldo,
                    int num_cus, hipStream_t st) {
    constexpr int lds = GemmB2::LDS_BYTES + kPersistBiasMax * 4 + 8 * 2048;  // slots + bias + per-wave epilogue scratch
    const int grid = num_cus / 8 * 8;
    { int rc_ = ensure_dynamic_lds((const void*)gemm_big_kernel<EPI>, lds); if (rc_) return rc_; }
    hipLaunchKernelGGL((gemm_big_kernel<EPI>), dim3(grid), dim3(512), lds, st, A, lda, W, bias, M_cap, M_dev, N, K, out, ldo);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

template <int EPI>
int launch_gemm_quad(const _Float16* A, int lda, const _Float16* W, const float* bias, int M_cap, const int* M_dev, int N, int K, void* out, int ldo,
                     int num_cus, hipStream_t st) {
    constexpr int lds = GemmB2::LDS_BYTES + kPersistBiasMax * 4 + 4 * 4096;  // slots + bias + per-wave epilogue scratch
    const int grid = num_cus / 8 * 8;
    { int rc_ = ensure_dynamic_lds((const void*)gemm_quad_kernel<EPI>, lds); if (rc_) return rc_; }
    hipLaunchKernelGGL((gemm_quad_kernel<EPI>), dim3(grid), dim3(256), lds, st, A, lda, W, bias, M_cap, M_dev, N, K, out, ldo);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

// The kernel is gemm_choose's (csrc/mdr_gemm_choice.h); M_est: expected number of valid rows (the packed token count is only known on the device).
// *res_added tells the caller whether the residual went into the output (else the following LayerNorm adds it).
template <int EPI>
int launch_gemm(const _Float16* A, int lda, const _Float16* W, const float* bias, int M_cap, const int* M_dev, int N, int K, void* out, int ldo,
                const _Float16* res, int ldr, int M_est, int num_cus, hipStream_t st, bool* res_added = nullptr, int force = -1) {
    // K: any multiple of 64 from 64 on for the one-tile kernel (2 to 4 stages), gemm_tail_tile, gemm_persist_kernel and gemm_big_kernel -- their prologues
    // skip the stages past K / 64, their counted waits never allow more batches in flight than were issued (the persistent kernels issue surplus batches so
    // that the count is constant) and a tile's pending stores are flushed when the next tile has fewer K-steps than pairs of fragments; the four-wave kernel
    // needs an even K / 64 >= 4 and gemm_choose routes around it.
    static int env_sel = getenv("MDR_GEMM_CFG") ? atoi(getenv("MDR_GEMM_CFG")) : 0;  // experiment knob: gemm_choose's sel
    constexpr int E = EPI == EPI_BIAS_RES_F32 ? EPI_BIAS_F32 : EPI;  // what a persistent kernel runs: it leaves the residual to the caller
    const GemmChoice choice = gemm_choose(force >= 0 ? force : env_sel, force >= 0, M_cap, M_est, N, K, lda, ldo, E == EPI_BIAS_F32 ? 4 : 2, num_cus);
    if (res_added) *res_added = choice.res_added;
    else if (EPI == EPI_BIAS_RES_F32 && !choice.res_added)
        return set_error(MDR_E_STATE, "large-M GEMM with a residual needs the caller to take the residual (res_added)");
    switch (choice.kernel) {
    case 7: return launch_gemm_quad<E>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, num_cus, st);
    case 6: return launch_gemm_big<E>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, num_cus, st);
    case 4: return launch_gemm_persist<E, GemmP>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, num_cus, st);
    case 3: return launch_gemm_cfg<EPI, GemmBig>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr, st);
#ifdef MDR_GEMM_EXTRA_CFGS  // measurement builds: more tile shapes behind the test hook's kernel ids 8-13
    case 8: return launch_gemm_cfg<EPI, GemmCfg<128, 64, 2, 2, 3>>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr, st);
    case 9: return launch_gemm_cfg<EPI, GemmCfg<64, 128, 2, 2, 3>>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr, st);
    case 10: return launch_gemm_cfg<EPI, GemmCfg<128, 128, 2, 2, 3>>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr, st);
    case 11: return launch_gemm_cfg<EPI, GemmCfg<64, 64, 2, 2, 4>>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr, st);
    case 12: return launch_gemm_cfg<EPI, GemmCfg<128, 64, 4, 2, 3>>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr, st);
    case 13: return launch_gemm_cfg<EPI, GemmCfg<64, 64, 4, 2, 3>>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr, st);
#endif
    case 2: return launch_gemm_cfg<EPI, GemmMid>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr, st);
    default: return launch_gemm_cfg<EPI, GemmSmall>(A, lda, W, bias, M_cap, M_dev, N, K, out, ldo, res, ldr, st);
    }
}

template <int NT>
int launch_attention(const _Float16* qkv, const int* cu, int B, int L, int H, int heads, _Float16* ctx, hipStream_t st) {
    constexpr int lds = attention_lds_bytes<NT>();
    { int rc_ = ensure_dynamic_lds((const void*)attention_kernel<NT>, lds); if (rc_) return rc_; }
    dim3 grid(heads, B);
    hipLaunchKernelGGL((attention_kernel<NT>), grid, dim3(512), lds, st, qkv, cu, H, ctx);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int launch_attention_ring(const _Float16* qkv, const int* cu, const int* order, int B, int L, int H, int heads, _Float16* ctx, hipStream_t st) {
    { int rc_ = ensure_dynamic_lds((const void*)attention_ring_kernel, kRingLds); if (rc_) return rc_; }
    const int nblk = (L + 127) / 128;
    const long long pairs8 = ((long long)B * heads + 7) / 8 * 8;  // pairs rounded up to whole XCD rounds
    hipLaunchKernelGGL(attention_ring_kernel, dim3((unsigned)(pairs8 * nblk)), dim3(512), kRingLds, st, qkv, cu, order, B, heads, nblk, H, ctx);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

template <int NTC>
int launch_attention_stream(const _Float16* qkv, const int* cu, const int* order, int B, int L, int H, int heads, _Float16* ctx, hipStream_t st) {
    if (MDR_ATTN_RING) return launch_attention_ring(qkv, cu, order, B, L, H, heads, ctx, st);  // (the product; MDR_ATTN_RING=0 builds: the streaming kernel)
    constexpr int lds = NTC * 16 * 128 * 2;
    { int rc_ = ensure_dynamic_lds((const void*)attention_stream_kernel<NTC>, lds); if (rc_) return rc_; }
    dim3 grid(heads, B, (L + 127) / 128);
    hipLaunchKernelGGL((attention_stream_kernel<NTC>), grid, dim3(kAttnThreads), lds, st, qkv, cu, H, ctx);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

// The ONE place that maps the padded length L of a batch to an attention kernel: mdr_encoder_forward, mdr_reader_forward and the mdr_test_attention
// hook all come through here. sel: 0 (product) = by length -- the one-shot kernel up to 128 tokens, the ring kernel above; 1 = the one-shot kernel, NT from L
// (the hook, and MDR_ATTN_FORCE=1 measurement builds); 2 = the ring kernel (MDR_ATTN_RING=0 measurement builds: the streaming kernel, chunk size from L).
constexpr int kOneShotMaxL = 32 * 16;  // keys the largest one-shot instantiation holds
int launch_attention_for(int sel, const _Float16* qkv, const int* cu, const int* order, int B, int L, int H, int heads, _Float16* ctx, hipStream_t st) {
    if (sel == 2 || (sel == 0 && L > 128))
        return L <= 64 ? launch_attention_stream<4>(qkv, cu, order, B, L, H, heads, ctx, st) : launch_attention_stream<16>(qkv, cu, order, B, L, H, heads, ctx, st);
    if (L <= 128) return launch_attention<8>(qkv, cu, B, L, H, heads, ctx, st);
    if (L <= 384) return launch_attention<24>(qkv, cu, B, L, H, heads, ctx, st);
    return launch_attention<32>(qkv, cu, B, L, H, heads, ctx, st);
}

}  // namespace

#include "mdr_encoder_trunk.inl"

struct mdr_encoder {
    Trunk t;  // t.type: row 0 of the token-type table (type_vocab == 1 for RoBERTa)
    _Float16* wproj = nullptr;
    float *bproj = nullptr, *lnp_g = nullptr, *lnp_b = nullptr;
    float fill_hint = 0.f;  // expected (tokens / (batch * seq_len)) of the next forwards; 0 = unknown (2/3 is assumed)
};

namespace {

// the encoder's embedding launch (RoBERTa position ids from tok_pid, one type row): one wave per packed token, cap = batch * seq_len waves launched
void launch_embed_ln(const long long* ids, const int* tok_src, const int* tok_pid, const int* total, int cap, const float* word, const float* pos,
                     const float* type0, const float* g, const float* b, int H, int vocab, int max_pos, float eps, _Float16* out16, float* out32,
                     hipStream_t st, const DropoutParams* drop = nullptr) {
    if (drop)  // y * m, then the fp16 copy of the masked value (mdr_encoder_dropout.inl)
        hipLaunchKernelGGL(embed_ln_dropout_kernel, dim3((cap + 3) / 4), dim3(256), 0, st, ids, tok_src, tok_pid, total, word, pos, type0, g, b, H, vocab,
                           max_pos, eps, *drop, out16, out32);
    else
        hipLaunchKernelGGL(embed_ln_kernel, dim3((cap + 3) / 4), dim3(256), 0, st, ids, tok_src, tok_pid, total, word, pos, type0, g, b, H, vocab, max_pos,
                           eps, out16, out32);
}

// What the GEMM test hooks ask of their integers. mdr_test_gemm_f16 has no epilogue 2 and, in MDR_GEMM_EXTRA_CFGS builds, the kernels 8-13.
int check_gemm_hook_args(int M, int M_est, int N, int K, int epilogue, int kernel, bool f16_hook) {
    MDR_REQUIRE(M > 0 && N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0, "bad GEMM shape M=%d N=%d K=%d (N, K multiples of 64)", M, N, K);
    MDR_REQUIRE(M_est >= 1, "M_est=%d must be at least 1", M_est);
    if (f16_hook) MDR_REQUIRE(epilogue == EPI_BIAS_F16 || epilogue == EPI_BIAS_GELU_F16 || epilogue == EPI_BIAS_F32, "epilogue must be 0, 1 or 3");
    MDR_REQUIRE(epilogue >= EPI_BIAS_F16 && epilogue <= EPI_BIAS_F32, "epilogue must be 0, 1, 2 or 3");
    const bool product_kernel = kernel == 0 || kernel == 1 || kernel == 2 || kernel == 4 || kernel == 6 || kernel == 7;
#ifdef MDR_GEMM_EXTRA_CFGS
    if (f16_hook) MDR_REQUIRE(product_kernel || (kernel >= 8 && kernel <= 13), "kernel must be 0, 1, 2, 4, 6, 7 or 8-13");
    else
#endif
    MDR_REQUIRE(product_kernel, "kernel must be 0, 1, 2, 4, 6 or 7");
    return MDR_OK;
}

// mdr_test_gemm_ex; mdr_test_gemm_f16 is this call with M_est = M, no residual and nobody to tell about it (f16_hook)
int test_gemm(const void* A_dev, const void* W_dev, const float* bias_dev, const void* res16_dev, int M, int M_est, const int* m_dev, int N, int K,
              void* out_dev, int epilogue, int kernel, int* res_added_host, bool f16_hook, int device, void* stream) {
    MDR_REQUIRE(A_dev && W_dev && bias_dev && out_dev, "NULL pointer");
    if (int rc = check_gemm_hook_args(M, M_est, N, K, epilogue, kernel, f16_hook)) return rc;
    MDR_REQUIRE((epilogue == EPI_BIAS_RES_F32) == (res16_dev != nullptr), "res16_dev goes with epilogue 2 and with no other");
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    const int ncu = device_cu_count(device);
    const _Float16* A = (const _Float16*)A_dev;
    const _Float16* W = (const _Float16*)W_dev;
    const _Float16* res = (const _Float16*)res16_dev;
    hipStream_t st = (hipStream_t)stream;
    bool added = true;
    bool* ra = res_added_host ? &added : nullptr;
    int rc;
    if (epilogue == EPI_BIAS_F16) rc = launch_gemm<EPI_BIAS_F16>(A, K, W, bias_dev, M, m_dev, N, K, out_dev, N, nullptr, 0, M_est, ncu, st, ra, kernel);
    else if (epilogue == EPI_BIAS_GELU_F16) rc = launch_gemm<EPI_BIAS_GELU_F16>(A, K, W, bias_dev, M, m_dev, N, K, out_dev, N, nullptr, 0, M_est, ncu, st, ra, kernel);
    else if (epilogue == EPI_BIAS_RES_F32) rc = launch_gemm<EPI_BIAS_RES_F32>(A, K, W, bias_dev, M, m_dev, N, K, out_dev, N, res, N, M_est, ncu, st, ra, kernel);
    else rc = launch_gemm<EPI_BIAS_F32>(A, K, W, bias_dev, M, m_dev, N, K, out_dev, N, nullptr, 0, M_est, ncu, st, ra, kernel);
    if (res_added_host) *res_added_host = added ? 1 : 0;
    return rc;
}

}  // namespace

static int encoder_forward(mdr_encoder* h, const int64_t* ids_dev, const int64_t* mask_dev, int batch, int seq_len, const TrunkDropout* drop,
                           float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

extern "C" {

int mdr_encoder_create(const mdr_encoder_config* cfg, const mdr_tensor* tensors, int n_tensors, int weights_on_device, int device, void* stream,
                       mdr_encoder** out) {
    MDR_REQUIRE(cfg && tensors && out, "NULL argument");
    MDR_REQUIRE(cfg->max_pos > 2, "bad geometry");
    if (int rc = trunk_check(*cfg, device)) return rc;
    DeviceGuard guard(device);
    mdr_encoder* h = new (std::nothrow) mdr_encoder();
    MDR_REQUIRE(h != nullptr, "out of host memory");
    const size_t H = cfg->hidden;
    WeightLoader ld{tensors, n_tensors, weights_on_device, (hipStream_t)stream, &h->t.allocs};
    trunk_upload(h->t, *cfg, device, 1, ld);
    ld.keep16("project.0.weight", H * H, &h->wproj);
    ld.keep32("project.0.bias", H, &h->bproj);
    ld.keep32("project.1.weight", H, &h->lnp_g);
    ld.keep32("project.1.bias", H, &h->lnp_b);
    if (int rc = ld.finish()) {
        mdr_encoder_free(h);
        return rc;
    }
    *out = h;
    return MDR_OK;
}

int mdr_test_gemm_f16(const void* A_dev, const void* W_dev, const float* bias_dev, int M, const int* m_dev, int N, int K, void* out_dev, int epilogue,
                      int kernel, int device, void* stream) {
    return test_gemm(A_dev, W_dev, bias_dev, nullptr, M, M, m_dev, N, K, out_dev, epilogue, kernel, nullptr, true, device, stream);
}

int mdr_test_gemm_ex(const void* A_dev, const void* W_dev, const float* bias_dev, const void* res16_dev, int M, int M_est, const int* m_dev, int N, int K,
                     void* out_dev, int epilogue, int kernel, int* res_added_host, int device, void* stream) {
    return test_gemm(A_dev, W_dev, bias_dev, res16_dev, M, M_est, m_dev, N, K, out_dev, epilogue, kernel, res_added_host, false, device, stream);
}

int mdr_test_gemm_choice(int kernel, int M, int M_est, int N, int K, int epilogue, int num_cus, int* kernel_out, int* res_added_out,
                         int* walk_row_tiles_out) {
    if (int rc = check_gemm_hook_args(M, M_est, N, K, epilogue, kernel, false)) return rc;
    MDR_REQUIRE(num_cus >= 8, "num_cus=%d must be at least 8", num_cus);
    const GemmChoice c = gemm_choose(kernel, kernel != 0, M, M_est, N, K, K, N, epilogue == EPI_BIAS_RES_F32 || epilogue == EPI_BIAS_F32 ? 4 : 2, num_cus);
    if (kernel_out) *kernel_out = c.kernel;
    if (res_added_out) *res_added_out = c.res_added ? 1 : 0;
    if (walk_row_tiles_out) {
        const int grid = num_cus / 8 * 8, ntm_all = (M_est + 255) / 256;
        *walk_row_tiles_out = c.kernel == 6   ? gemm_head_row_tiles(ntm_all, N / 256, grid, grid / 2)  // (gemm_big_kernel's call,
                              : c.kernel == 7 ? gemm_head_row_tiles(ntm_all, N / 256, grid, grid / 4)  //  gemm_quad_kernel's)
                              : c.kernel == 4 ? ntm_all
                                              : 0;
    }
    return MDR_OK;
}

int mdr_test_attention(const void* qkv_dev, const int* cu_dev, const int* order_dev, int B, int L, int hidden, int heads, int kernel, void* ctx_dev,
                       int device, void* stream) {
    MDR_REQUIRE(qkv_dev && cu_dev && ctx_dev, "NULL pointer");
    MDR_REQUIRE(B >= 1, "B=%d must be at least 1", B);
    MDR_REQUIRE(L >= 1 && L <= 512, "L=%d out of range (1..512)", L);
    MDR_REQUIRE(heads >= 1 && hidden == 64 * heads, "head dim must be 64 (hidden=%d heads=%d)", hidden, heads);
    MDR_REQUIRE(kernel >= 0 && kernel <= 3, "kernel must be 0, 1, 2 or 3");
    MDR_REQUIRE(kernel != 1 || L <= kOneShotMaxL, "kernel 1 (one-shot) holds at most %d keys, L=%d", kOneShotMaxL, L);
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    const _Float16* qkv = (const _Float16*)qkv_dev;
    hipStream_t st = (hipStream_t)stream;
    if (kernel == 3) {  // (the launch of mdr_encoder_forward's last layer)
        hipLaunchKernelGGL(attention_cls_kernel, dim3(heads, B), dim3(64), 0, st, qkv, cu_dev, hidden, (_Float16*)ctx_dev);
        MDR_HIP_TRY(hipGetLastError());
        return MDR_OK;
    }
    return launch_attention_for(kernel, qkv, cu_dev, order_dev, B, L, hidden, heads, (_Float16*)ctx_dev, st);
}

#if MDR_GEMM_ABL == 5  // measurement builds only (include/mdr_hip_measure.h)
int mdr_test_gemm_stamps(unsigned long long* out8_host, int reset) {
    MDR_REQUIRE(out8_host, "NULL pointer");
    MDR_HIP_TRY(hipDeviceSynchronize());
    MDR_HIP_TRY(hipMemcpyFromSymbol(out8_host, HIP_SYMBOL(g_gemm_stamp), 8 * sizeof(unsigned long long)));
    if (reset) {
        const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        MDR_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_stamp), z, sizeof(z)));
    }
    return MDR_OK;
}
#endif

#if MDR_ATTN_ABL == 9  // measurement builds only (include/mdr_hip_measure.h)
int mdr_test_attn_stamps(unsigned long long* out_host, int max_wgs) {
    MDR_REQUIRE(out_host && max_wgs > 0 && max_wgs <= kAttnStampWgs, "NULL pointer or max_wgs out of range");
    MDR_HIP_TRY(hipDeviceSynchronize());
    MDR_HIP_TRY(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_attn_stamp), (size_t)max_wgs * 8 * sizeof(unsigned long long)));
    return MDR_OK;
}
#endif

#if MDR_CU_LANES  // measurement builds only (include/mdr_hip_measure.h): CU-partitioned lanes, a measured negative of round 5
static std::mutex g_cu_mu;
static std::map<hipStream_t, int> g_stream_cus;  // CUs a stream may use, read at its first un-captured forward
int mdr_stream_create_cu_range(int device, int cu_lo, int cu_hi, void** stream_out) {
    MDR_REQUIRE(stream_out != nullptr, "stream_out is NULL");
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    hipDeviceProp_t prop;
    MDR_HIP_TRY(hipGetDeviceProperties(&prop, device));
    const int n = prop.multiProcessorCount;
    MDR_REQUIRE(cu_lo >= 0 && cu_hi <= n && cu_hi - cu_lo >= 8 && cu_lo % 8 == 0 && cu_hi % 8 == 0, "CU range [%d, %d) must be multiples of 8 inside [0, %d)", cu_lo,
                cu_hi, n);
    std::vector<uint32_t> mask((size_t)(n + 31) / 32, 0u);
    for (int i = cu_lo; i < cu_hi; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
    hipStream_t st = nullptr;
    MDR_HIP_TRY(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
    *stream_out = (void*)st;
    return MDR_OK;
}

int mdr_stream_destroy(void* stream) {
    {
        std::lock_guard<std::mutex> lk(g_cu_mu);
        g_stream_cus.erase((hipStream_t)stream);
    }
    if (stream) MDR_HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return MDR_OK;
}
#endif

int mdr_encoder_set_fill_hint(mdr_encoder* h, float fill) {
    MDR_REQUIRE(h != nullptr, "encoder handle is NULL");
    MDR_REQUIRE(fill >= 0.f && fill <= 1.f, "fill must be in [0, 1] (0 = unknown)");
    h->fill_hint = fill;
    return MDR_OK;
}

int mdr_encoder_free(mdr_encoder* h) {
    if (!h) return MDR_OK;
    trunk_free(h->t);
    delete h;
    return MDR_OK;
}

size_t mdr_encoder_workspace_bytes(const mdr_encoder* h, int batch, int seq_len) {
    if (!h || batch <= 0 || seq_len <= 0) return 0;
    return carve(h->t.cfg, batch, seq_len, nullptr).bytes;
}

int mdr_encoder_forward(mdr_encoder* h, const int64_t* ids_dev, const int64_t* mask_dev, int batch, int seq_len, float* out_dev, void* workspace_dev,
                        size_t workspace_bytes, void* stream) {
    return encoder_forward(h, ids_dev, mask_dev, batch, seq_len, nullptr, out_dev, workspace_dev, workspace_bytes, stream);
}

}  // extern "C"

// mdr_encoder_forward (drop == nullptr) and mdr_encoder_forward_dropout (mdr_encoder_dropout_api.inl): one launch sequence, the dropout
// places live where drop's thresholds are not 0
static int encoder_forward(mdr_encoder* h, const int64_t* ids_dev, const int64_t* mask_dev, int batch, int seq_len, const TrunkDropout* drop,
                           float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    MDR_REQUIRE(h != nullptr, "encoder handle is NULL");
    MDR_REQUIRE(batch >= 0 && seq_len > 0, "bad shape batch=%d seq_len=%d", batch, seq_len);
    if (batch == 0) return MDR_OK;
    MDR_REQUIRE(ids_dev && mask_dev && out_dev, "NULL pointer");
    MDR_REQUIRE(seq_len <= 512, "seq_len=%d exceeds 512 (RoBERTa has 514 positions)", seq_len);
    MDR_REQUIRE((long long)batch * seq_len < (1ll << 31), "batch*seq_len overflows int32; split the batch");
    const Trunk& t = h->t;
    const mdr_encoder_config& c = t.cfg;
    DeviceGuard guard(t.device);
    hipStream_t st = (hipStream_t)stream;
    const long long* ids = (const long long*)ids_dev;
    Workspace w;
    if (int rc = trunk_begin(t, ids, (const long long*)mask_dev, batch, seq_len, workspace_dev, workspace_bytes, carve(c, batch, seq_len, nullptr).bytes, st, &w))
        return rc;
    const int B = batch, L = seq_len, H = c.hidden;
    const int Tcap = B * L;
    // tile-shape heuristics only: the packed token count is known on the device; the host may pass what it expects
    const int Test = h->fill_hint > 0.f ? std::max(1, (int)(h->fill_hint * (float)Tcap)) : Tcap - Tcap / 3;
    int ncu = t.num_cus;
#if MDR_CU_LANES
    {  // CU-partitioned lanes (measurement build): the persistent GEMMs size their grids for the CUs THIS stream may run on. The mask cannot be read while the
       // stream is capturing, so the count of the warm-up call on the same stream is remembered (erased by mdr_stream_destroy); only MASKED streams are rounded
       // to whole XCD shares
        std::lock_guard<std::mutex> lk(g_cu_mu);
        auto it = g_stream_cus.find(st);
        if (it != g_stream_cus.end()) ncu = it->second;
        else {
            uint32_t mask[32] = {0};
            int n = 0;
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone && hipExtStreamGetCUMask(st, 32, mask) == hipSuccess)
                for (uint32_t w_ : mask) n += __builtin_popcount(w_);
            else (void)hipGetLastError();
            if (n >= 8 && n < t.num_cus) ncu = n / 8 * 8;
            if (cs == hipStreamCaptureStatusNone) g_stream_cus[st] = ncu;
        }
    }
#endif
    const bool drop_hid = drop && drop->T_hidden, drop_att = drop && drop->T_attention;
    const DropoutParams emb_drop = drop_hid ? drop->params(0, kPlaceEmb) : DropoutParams{};
    launch_embed_ln(ids, w.tok_src, w.tok_pid, w.total, Tcap, t.word, t.pos, t.type, t.emb_g, t.emb_b, H, c.vocab, c.max_pos, c.ln_eps, w.h16, w.h32, st,
                    drop_hid ? &emb_drop : nullptr);
    MDR_HIP_TRY(hipGetLastError());
    const Rows tokens{w.h16, w.h32, w.pre, Tcap, w.total, Test}, cls{w.cls16, w.cls32, w.clspre, B, nullptr, B};
    int rc;
    for (int i = 0; i + 1 < c.layers; ++i) {
        rc = trunk_layer(t, t.layers[i], w, tokens, B, L, ncu, st, drop, i);
        if (rc) return rc;
    }
    // ---- last layer: everything after the K/V projection only for the CLS rows ([B, H] instead of [T, H]) ----
    const Layer& last = t.layers.back();
    rc = launch_qkv(t, last, w, tokens, ncu, st);
    if (rc) return rc;
    launch_gather_cls(w.h16, w.h32, w.cu, B, H, w.cls16, w.cls32, st);
    const int li = c.layers - 1;
    if (drop_att) {  // the first query of each sequence under the attention mask (mode 3 of include/mdr_dropout.h)
        rc = mdr_attention_dropout_forward(w.qkv, w.cu, B, L, H, c.heads, 3, (int)drop->T_attention, drop->seed, drop->site(li, kPlaceAttn), w.ctx, t.device,
                                           stream);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(attention_cls_kernel, dim3(c.heads, B), dim3(64), 0, st, (const _Float16*)w.qkv, (const int*)w.cu, H, w.ctx);
        MDR_HIP_TRY(hipGetLastError());
    }
    rc = layer_tail(t, last, w.ctx, w.ffn, cls, ncu, st, drop, li);
    if (rc) return rc;
    rc = launch_gemm<EPI_BIAS_F32>(w.cls16, H, h->wproj, h->bproj, B, nullptr, H, H, w.clspre, H, nullptr, 0, B, ncu, st);
    if (rc) return rc;
    launch_layernorm((const float*)w.clspre, (const _Float16*)nullptr, (const float*)nullptr, B, (const int*)nullptr, H, h->lnp_g, h->lnp_b, c.ln_eps,
                     (_Float16*)nullptr, out_dev, st);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

// the answer reader (include/mdr_reader.h) shares this translation unit's file-local kernels and launchers
#include "mdr_reader.inl"
#include "mdr_reader_assemble.inl"
// the mdr_test_* hooks of the packing / embedding / LayerNorm / row kernels (behind the reader: its embedding kernel is one of them)
#include "mdr_encoder_test_rows.inl"
// the training-mode forward and the test hooks of its two row kernels (include/mdr_encoder_dropout.h)
#include "mdr_encoder_dropout_api.inl"
// the backward of the trunk's Linears (include/mdr_linear_grad.h): its dX goes through launch_gemm
#include "mdr_linear_grad.inl"
