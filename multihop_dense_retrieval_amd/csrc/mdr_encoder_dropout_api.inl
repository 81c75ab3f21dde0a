// csrc/mdr_encoder_dropout_api.inl -- entry points of include/mdr_encoder_dropout.h: the training-mode forward of the inference encoder and
// the test hooks of its two row kernels (mdr_encoder_dropout.inl). Included by mdr_encoder.hip behind encoder_forward, which is the launch
// sequence; what is here validates on the host. Not a translation unit of its own.

extern "C" {

int mdr_encoder_forward_dropout(mdr_encoder* h, const int64_t* ids_dev, const int64_t* mask_dev, int batch, int seq_len, int T_hidden, int T_attention,
                                uint64_t seed, int encode, float* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* fn = "mdr_encoder_forward_dropout";
    MDR_REQUIRE(h != nullptr, "%s: encoder handle is NULL", fn);
    MDR_REQUIRE(h->t.cfg.residual_fp32 == 2, "%s: built for residual_fp32 = 2 only (the mode training runs in), this handle has %d", fn,
                h->t.cfg.residual_fp32);
    MDR_REQUIRE(T_hidden >= 0 && T_hidden <= 255 && T_attention >= 0 && T_attention <= 255, "%s: T_hidden=%d T_attention=%d out of range (0..255)", fn,
                T_hidden, T_attention);
    MDR_REQUIRE(encode >= 0 && encode < kDropoutEncodes, "%s: encode=%d out of range (0..%d)", fn, encode, kDropoutEncodes - 1);
    MDR_REQUIRE(h->t.cfg.layers <= kDropoutMaxLayers, "%s: %d layers, the site formula holds %d", fn, h->t.cfg.layers, kDropoutMaxLayers);
    MDR_REQUIRE(batch <= 65535, "%s: batch=%d out of range (the attention mask's sequence index, <= 65535)", fn, batch);
    const TrunkDropout drop{(unsigned)T_hidden, (unsigned)T_attention, seed, encode};
    return encoder_forward(h, ids_dev, mask_dev, batch, seq_len, T_hidden || T_attention ? &drop : nullptr, out_dev, workspace_dev, workspace_bytes, stream);
}

int mdr_test_layernorm_dropout(const void* in16_dev, const float* res32_dev, int rows_cap, const int* rows_dev, int H, const float* g_dev,
                               const float* b_dev, float eps, int T, uint64_t seed, uint32_t site, void* out16_dev, float* out32_dev, int device,
                               void* stream) {
    MDR_REQUIRE(in16_dev && g_dev && b_dev, "NULL pointer");
    MDR_REQUIRE(out16_dev || out32_dev, "NULL pointer (out16 and out32)");
    MDR_REQUIRE(rows_cap >= 1, "rows_cap=%d must be at least 1", rows_cap);
    MDR_REQUIRE(rows_hidden_ok(H), "H=%d unsupported (multiple of 64, <= 1024)", H);
    MDR_REQUIRE(T >= 0 && T <= 255, "T=%d out of range (0..255)", T);
    MDR_REQUIRE(aligned16({in16_dev, res32_dev, g_dev, b_dev, out16_dev, out32_dev}), "pointers must be 16-byte aligned");
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    launch_layernorm_dropout((const _Float16*)in16_dev, res32_dev, rows_cap, rows_dev, H, g_dev, b_dev, eps, dropout_params((unsigned)T, seed, site),
                             (_Float16*)out16_dev, out32_dev, (hipStream_t)stream);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int mdr_test_embed_ln_dropout(const int64_t* ids_dev, const int* tok_src_dev, const int* tok_pid_dev, const int* total_dev, int cap,
                              const float* word_dev, const float* pos_dev, const float* type_dev, const float* g_dev, const float* b_dev, int H,
                              int vocab, int max_pos, float eps, int T, uint64_t seed, uint32_t site, void* out16_dev, float* out32_dev, int device,
                              void* stream) {
    MDR_REQUIRE(ids_dev && tok_src_dev && tok_pid_dev && total_dev && word_dev && pos_dev && type_dev && g_dev && b_dev && out16_dev, "NULL pointer");
    MDR_REQUIRE(cap >= 1, "cap=%d must be at least 1", cap);
    MDR_REQUIRE(rows_hidden_ok(H), "H=%d unsupported (multiple of 64, <= 1024)", H);
    MDR_REQUIRE(vocab >= 1 && max_pos >= 1, "bad table sizes vocab=%d max_pos=%d", vocab, max_pos);
    MDR_REQUIRE(T >= 0 && T <= 255, "T=%d out of range (0..255)", T);
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    const DropoutParams dp = dropout_params((unsigned)T, seed, site);
    launch_embed_ln((const long long*)ids_dev, tok_src_dev, tok_pid_dev, total_dev, cap, word_dev, pos_dev, type_dev, g_dev, b_dev, H, vocab, max_pos, eps,
                    (_Float16*)out16_dev, out32_dev, (hipStream_t)stream, &dp);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // extern "C"
