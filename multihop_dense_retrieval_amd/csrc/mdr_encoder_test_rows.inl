// csrc/mdr_encoder_test_rows.inl -- test hooks (include/mdr_hip.h) of the trunk's packing, embedding, LayerNorm and row kernels, each in isolation.
// Included at the end of mdr_encoder.hip; not a translation unit of its own. No kernels and no launches of its own here: every hook validates
// its arguments on the host and goes through the launcher the forwards use (launch_pack, launch_embed_ln, launch_reader_embed_ln,
// launch_layernorm, launch_gather_cls, launch_f32_to_f16), so what a test sees is the grid, block and argument order of the product.

namespace {

bool rows_hidden_ok(int H) { return H >= 64 && H <= 64 * kMaxPerLane && H % 64 == 0; }

}  // namespace

extern "C" {

int mdr_test_pack(const int64_t* ids_dev, const int64_t* mask_dev, int B, int L, int pad_id, int* lens_dev, int* cu_dev, int* total_dev, int* order_dev,
                  int* tok_src_dev, int* tok_pid_dev, int device, void* stream) {
    MDR_REQUIRE(ids_dev && mask_dev && lens_dev && cu_dev && total_dev && order_dev && tok_src_dev && tok_pid_dev, "NULL pointer");
    MDR_REQUIRE(B >= 1, "B=%d must be at least 1", B);
    MDR_REQUIRE(L >= 1 && L <= 512, "L=%d out of range (1..512)", L);
    MDR_REQUIRE((long long)B * L < (1ll << 31), "B*L overflows int32 (B=%d L=%d)", B, L);
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    launch_pack((const long long*)ids_dev, (const long long*)mask_dev, B, L, pad_id, lens_dev, cu_dev, total_dev, order_dev, tok_src_dev, tok_pid_dev,
                (hipStream_t)stream);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int mdr_test_embed_ln(int flavour, const int64_t* ids_dev, const int64_t* types_dev, const int* tok_src_dev, const int* tok_pid_dev, const int* total_dev,
                      int cap, int L, const float* word_dev, const float* pos_dev, const float* type_dev, int type_vocab, const float* g_dev,
                      const float* b_dev, int H, int vocab, int max_pos, float eps, void* out16_dev, float* out32_dev, int device, void* stream) {
    MDR_REQUIRE(flavour == 0 || flavour == 1, "flavour must be 0 (RoBERTa) or 1 (reader)");
    MDR_REQUIRE(ids_dev && tok_src_dev && total_dev && word_dev && pos_dev && type_dev && g_dev && b_dev && out16_dev, "NULL pointer");
    MDR_REQUIRE(flavour == 1 || tok_pid_dev, "NULL pointer (tok_pid)");
    MDR_REQUIRE(cap >= 1, "cap=%d must be at least 1", cap);
    MDR_REQUIRE(rows_hidden_ok(H), "H=%d unsupported (multiple of 64, <= 1024)", H);
    MDR_REQUIRE(vocab >= 1 && max_pos >= 1, "bad table sizes vocab=%d max_pos=%d", vocab, max_pos);
    MDR_REQUIRE(flavour == 0 || (L >= 1 && L <= 512 && L <= max_pos), "L=%d out of range (1..min(512, max_pos=%d))", L, max_pos);
    MDR_REQUIRE(flavour == 0 || type_vocab >= 1, "type_vocab=%d must be at least 1", type_vocab);
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    const long long* ids = (const long long*)ids_dev;
    if (flavour == 0)
        launch_embed_ln(ids, tok_src_dev, tok_pid_dev, total_dev, cap, word_dev, pos_dev, type_dev, g_dev, b_dev, H, vocab, max_pos, eps, (_Float16*)out16_dev,
                        out32_dev, (hipStream_t)stream);
    else
        launch_reader_embed_ln(ids, (const long long*)types_dev, tok_src_dev, total_dev, cap, L, word_dev, pos_dev, type_dev, type_vocab, g_dev, b_dev, H, vocab,
                               eps, (_Float16*)out16_dev, out32_dev, (hipStream_t)stream);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int mdr_test_layernorm(const void* in_dev, int in_f16, const void* res16_dev, const float* res32_dev, int rows_cap, const int* rows_dev, int H,
                       const float* g_dev, const float* b_dev, float eps, void* out16_dev, float* out32_dev, int device, void* stream) {
    MDR_REQUIRE(in_dev && g_dev && b_dev, "NULL pointer");
    MDR_REQUIRE(out16_dev || out32_dev, "NULL pointer (out16 and out32)");
    MDR_REQUIRE(!(res16_dev && res32_dev), "at most one of res16 / res32");
    MDR_REQUIRE(in_f16 == 0 || in_f16 == 1, "in_f16 must be 0 or 1");
    MDR_REQUIRE(rows_cap >= 1, "rows_cap=%d must be at least 1", rows_cap);
    MDR_REQUIRE(rows_hidden_ok(H), "H=%d unsupported (multiple of 64, <= 1024)", H);
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    if (in_f16)
        launch_layernorm((const _Float16*)in_dev, (const _Float16*)res16_dev, res32_dev, rows_cap, rows_dev, H, g_dev, b_dev, eps, (_Float16*)out16_dev,
                         out32_dev, (hipStream_t)stream);
    else
        launch_layernorm((const float*)in_dev, (const _Float16*)res16_dev, res32_dev, rows_cap, rows_dev, H, g_dev, b_dev, eps, (_Float16*)out16_dev,
                         out32_dev, (hipStream_t)stream);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int mdr_test_row_copy(int mode, const void* src16_dev, const float* src32_dev, const int* cu_dev, int B, int H, int64_t n, void* out16_dev,
                      float* out32_dev, int device, void* stream) {
    MDR_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (CLS gather) or 1 (f32 -> f16)");
    if (mode == 0) {
        MDR_REQUIRE(src16_dev && cu_dev && out16_dev, "NULL pointer");
        MDR_REQUIRE(!src32_dev == !out32_dev, "NULL pointer (src32 and out32 go together)");
        MDR_REQUIRE(B >= 1, "B=%d must be at least 1", B);
        MDR_REQUIRE(rows_hidden_ok(H), "H=%d unsupported (multiple of 64, <= 1024)", H);
    } else {
        MDR_REQUIRE(src32_dev && out16_dev, "NULL pointer");
        MDR_REQUIRE(n >= 1 && n < (256ll << 31), "n=%lld out of range", (long long)n);
    }
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    if (mode == 0)
        launch_gather_cls((const _Float16*)src16_dev, src32_dev, cu_dev, B, H, (_Float16*)out16_dev, out32_dev, (hipStream_t)stream);
    else
        launch_f32_to_f16(src32_dev, (_Float16*)out16_dev, (size_t)n, (hipStream_t)stream);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // extern "C"
