// csrc/mdr_encoder_trunk.inl -- host side of the BERT-style transformer trunk that the retrieval encoder (mdr_encoder.hip) and the answer
// reader (mdr_reader.inl) share: who owns the weights and how they are uploaded, the workspace and the packing prologue of a forward, and the
// layer body. Included by mdr_encoder.hip behind the GEMM / attention launchers; not a translation unit of its own. No kernels here.
//
// What differs between the two models stays with them: the embedding kernel (RoBERTa position ids and one type row against absolute positions
// and a type table), the encoder's CLS-only last layer and projection head, the reader's pooler, heads and span search.

namespace {

struct Layer {
    _Float16 *wqkv, *wo, *w1, *w2;
    float *bqkv, *bo, *b1, *b2, *ln1_g, *ln1_b, *ln2_g, *ln2_b;
};

struct Trunk {
    mdr_encoder_config cfg{};  // geometry and residual mode (the reader fills it from its own config; pad_id is 0 there)
    int device = 0;
    int num_cus = 256;
    std::vector<void*> allocs;  // every device allocation of the handle, the owner's head weights included
    float *word = nullptr, *pos = nullptr, *type = nullptr, *emb_g = nullptr, *emb_b = nullptr;  // type: [type rows, H]
    std::vector<Layer> layers;
};

// ---- launchers of the packing / LayerNorm / row kernels: a forward and the mdr_test_* hooks of mdr_encoder_test_rows.inl both come through these, so
// that grid, block and argument order exist once ----

// lengths, cu_seqlens + total (+ the length order: written only where the ring attention kernel walks by it, B <= 1024 -- pack_order() says whether)
// and token -> (source index, RoBERTa position id)
inline int* pack_order(int* order, int B) { return MDR_ATTN_SORT && B <= 1024 ? order : nullptr; }
void launch_pack(const long long* ids, const long long* mask, int B, int L, int pad_id, int* lens, int* cu, int* total, int* order, int* tok_src,
                 int* tok_pid, hipStream_t st) {
    hipLaunchKernelGGL(enc_lens_kernel, dim3((B + 3) / 4), dim3(256), 0, st, mask, B, L, lens);
    hipLaunchKernelGGL(enc_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)lens, B, cu, total, pack_order(order, B));
    hipLaunchKernelGGL(enc_scatter_kernel, dim3((B + 3) / 4), dim3(256), 0, st, ids, mask, B, L, pad_id, (const int*)cu, tok_src, tok_pid);
}

template <typename IN_T>
void launch_layernorm(const IN_T* in, const _Float16* res16, const float* res32, int rows_cap, const int* rows_dev, int H, const float* g, const float* b,
                      float eps, _Float16* out16, float* out32, hipStream_t st) {
    hipLaunchKernelGGL(layernorm_kernel<IN_T>, dim3((rows_cap + 3) / 4), dim3(256), 0, st, in, res16, res32, rows_cap, rows_dev, H, g, b, eps, out16, out32);
}

// layernorm_kernel<_Float16> over fp32(fp16(fp32(in) * m)): the hidden-state dropout of a training-mode forward (mdr_encoder_dropout.inl)
void launch_layernorm_dropout(const _Float16* in, const float* res32, int rows_cap, const int* rows_dev, int H, const float* g, const float* b, float eps,
                              const DropoutParams& dp, _Float16* out16, float* out32, hipStream_t st) {
    hipLaunchKernelGGL(layernorm_dropout_kernel, dim3((rows_cap + 3) / 4), dim3(256), 0, st, in, res32, rows_cap, rows_dev, H, g, b, eps, dp, out16, out32);
}

// The dropout of one training-mode forward (include/mdr_encoder_dropout.h): the thresholds of the two kinds (0: that kind's places are
// plain), the step's seed and which of a step's encodes this is. The site of a place is dropout.site_of's:
//   site = 1 + (encode * 64 + layer) * 4 + place,   place: 0 emb (layer 0 only), 1 attn, 2 ao, 3 ff2
enum { kPlaceEmb = 0, kPlaceAttn = 1, kPlaceAo = 2, kPlaceFf2 = 3, kDropoutMaxLayers = 64, kDropoutEncodes = 6 };
struct TrunkDropout {
    unsigned T_hidden, T_attention;
    uint64_t seed;
    int encode;
    uint32_t site(int layer, int place) const { return 1u + ((uint32_t)encode * kDropoutMaxLayers + (uint32_t)layer) * 4u + (uint32_t)place; }
    DropoutParams params(int layer, int place) const { return dropout_params(place == kPlaceAttn ? T_attention : T_hidden, seed, site(layer, place)); }
};

void launch_gather_cls(const _Float16* h16, const float* h32, const int* cu, int B, int H, _Float16* out16, float* out32, hipStream_t st) {
    hipLaunchKernelGGL(gather_cls_kernel, dim3((B * H + 255) / 256), dim3(256), 0, st, h16, h32, cu, B, H, out16, out32);
}

void launch_f32_to_f16(const float* in, _Float16* out, size_t numel, hipStream_t st) {
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, st, in, out, (long long)numel);
}

int device_cu_count(int device) {
    hipDeviceProp_t prop;
    return hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
}

// the checks both create functions make on the trunk's geometry and on the device
int trunk_check(const mdr_encoder_config& c, int device) {
    MDR_REQUIRE(c.hidden > 0 && c.hidden % 128 == 0 && c.hidden <= 1024, "hidden=%d unsupported (multiple of 128, <= 1024)", c.hidden);
    MDR_REQUIRE(c.heads > 0 && c.hidden == c.heads * 64, "head dim must be 64 (hidden=%d heads=%d)", c.hidden, c.heads);
    MDR_REQUIRE(c.ffn > 0 && c.ffn % 128 == 0, "ffn=%d must be a multiple of 128", c.ffn);
    MDR_REQUIRE(c.layers > 0 && c.vocab > 0 && c.max_pos > 0, "bad geometry");
    MDR_REQUIRE(c.residual_fp32 >= 0 && c.residual_fp32 <= 2, "residual_fp32=%d must be 0, 1 or 2", c.residual_fp32);
    int ndev = 0;
    MDR_HIP_TRY(hipGetDeviceCount(&ndev));
    MDR_REQUIRE(device >= 0 && device < ndev, "device %d out of range", device);
    return MDR_OK;
}

void trunk_free(Trunk& t) {
    DeviceGuard guard(t.device);
    for (void* p : t.allocs) (void)hipFree(p);
    t.allocs.clear();
}

const mdr_tensor* find_tensor(const mdr_tensor* ts, int n, const std::string& name) {
    for (int i = 0; i < n; ++i)
        if (ts[i].name && name == ts[i].name) return &ts[i];
    return nullptr;
}

// Uploads the fp32 tensors of a state dict by name (numel checked), host-to-device or device-to-device, as they are or converted to fp16
// through a staging buffer. The first failure sticks: every later call does nothing and returns its code (mdr_last_error() keeps its text), so a
// create function is a plain list of uploads with one check at the end. Allocations go on the handle's list and are freed with the handle; the
// staging buffer goes with the loader. `at`: element offset into dst. (create runs once: std::string and the heap are fine here.)
struct WeightLoader {
    const mdr_tensor* tensors;
    int n_tensors;
    int on_device;
    hipStream_t st;
    std::vector<void*>* allocs;
    float* staging = nullptr;
    int rc = MDR_OK;

    ~WeightLoader() {
        if (staging) (void)hipFree(staging);
    }
    int hip(hipError_t e, const char* what) {
        return e == hipSuccess ? MDR_OK : (rc = set_error(MDR_E_HIP, "%s failed: %s", what, hipGetErrorString(e)));
    }
    int stage(size_t elems) {
        if (rc) return rc;
        if (hipMalloc((void**)&staging, elems * 4) != hipSuccess) return rc = set_error(MDR_E_HIP, "hipMalloc(staging) failed");
        return MDR_OK;
    }
    int alloc(size_t bytes, void** p) {
        if (rc || hip(hipMalloc(p, bytes), "hipMalloc")) return rc;
        allocs->push_back(*p);
        return MDR_OK;
    }
    // `name` into device fp32 memory at dst + at
    int fetch32(const std::string& name, size_t numel, float* dst, size_t at = 0) {
        if (rc) return rc;
        const mdr_tensor* t = find_tensor(tensors, n_tensors, name);
        if (!t) return rc = set_error(MDR_E_INVALID, "missing key in state dict: %s", name.c_str());
        if ((size_t)t->numel != numel)
            return rc = set_error(MDR_E_INVALID, "size mismatch for %s: expected %zu elements, got %lld", name.c_str(), numel, (long long)t->numel);
        return hip(hipMemcpyAsync(dst + at, t->data, numel * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st), "hipMemcpyAsync");
    }
    int keep32(const std::string& name, size_t numel, float** dst) {
        alloc(numel * 4, (void**)dst);
        return fetch32(name, numel, *dst);
    }
    // staging[0, numel) -> fp16 at dst + at (the stream is drained: staging is reused)
    int convert16(size_t numel, _Float16* dst, size_t at = 0) {
        if (rc) return rc;
        launch_f32_to_f16(staging, dst + at, numel, st);
        if (hip(hipGetLastError(), "fp16 conversion launch")) return rc;
        return hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    }
    int to16(const std::string& name, size_t numel, _Float16* dst, size_t at = 0) {
        fetch32(name, numel, staging);
        return convert16(numel, dst, at);
    }
    int keep16(const std::string& name, size_t numel, _Float16** dst) {
        alloc(numel * 2, (void**)dst);
        return to16(name, numel, *dst);
    }
    int finish() {
        if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = set_error(MDR_E_HIP, "stream sync failed after weight upload");
        return rc;
    }
};

// Fills the trunk from cfg and uploads encoder.embeddings.* and encoder.encoder.layer.{i}.* ; type_rows: rows of the token-type table that are
// kept. The staging buffer holds the largest tensor that goes to fp16 on either side: an FFN or [H, H] matrix (the reader's [4, H] head block
// is smaller than both, ffn >= 128).
int trunk_upload(Trunk& t, const mdr_encoder_config& c, int device, int type_rows, WeightLoader& ld) {
    t.cfg = c;
    t.device = device;
    t.num_cus = device_cu_count(device);
    const size_t H = c.hidden, F = c.ffn;
    ld.stage(std::max(F * H, H * H));
    const std::string E = "encoder.embeddings.";
    ld.keep32(E + "word_embeddings.weight", (size_t)c.vocab * H, &t.word);
    ld.keep32(E + "position_embeddings.weight", (size_t)c.max_pos * H, &t.pos);
    ld.keep32(E + "token_type_embeddings.weight", (size_t)type_rows * H, &t.type);
    ld.keep32(E + "LayerNorm.weight", H, &t.emb_g);
    ld.keep32(E + "LayerNorm.bias", H, &t.emb_b);
    t.layers.resize(c.layers);
    for (int i = 0; i < c.layers; ++i) {
        Layer& Ly = t.layers[i];
        const std::string P = "encoder.encoder.layer." + std::to_string(i) + ".";
        ld.alloc(3 * H * H * 2, (void**)&Ly.wqkv);
        ld.alloc(3 * H * 4, (void**)&Ly.bqkv);
        const char* qkv_names[3] = {"query", "key", "value"};
        for (int j = 0; j < 3; ++j) {
            ld.to16(P + "attention.self." + qkv_names[j] + ".weight", H * H, Ly.wqkv, j * H * H);
            ld.fetch32(P + "attention.self." + qkv_names[j] + ".bias", H, Ly.bqkv, j * H);
        }
        ld.keep16(P + "attention.output.dense.weight", H * H, &Ly.wo);
        ld.keep32(P + "attention.output.dense.bias", H, &Ly.bo);
        ld.keep32(P + "attention.output.LayerNorm.weight", H, &Ly.ln1_g);
        ld.keep32(P + "attention.output.LayerNorm.bias", H, &Ly.ln1_b);
        ld.keep16(P + "intermediate.dense.weight", F * H, &Ly.w1);
        ld.keep32(P + "intermediate.dense.bias", F, &Ly.b1);
        ld.keep16(P + "output.dense.weight", H * F, &Ly.w2);
        ld.keep32(P + "output.dense.bias", H, &Ly.b2);
        ld.keep32(P + "output.LayerNorm.weight", H, &Ly.ln2_g);
        ld.keep32(P + "output.LayerNorm.bias", H, &Ly.ln2_b);
    }
    return ld.rc;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------------

struct Workspace {
    char* base;                                          // null when only the size is asked for
    int *lens, *cu, *total, *tok_src, *tok_pid, *order;  // order: sequences by length, longest first (the ring attention kernel's walk)
    _Float16 *h16, *qkv, *ctx, *ffn, *cls16;
    float *pre, *clspre, *h32, *cls32;  // h32 / cls32: the fp32 residual stream (residual_fp32 mode only)
    size_t bytes;
};

Workspace carve(const mdr_encoder_config& c, int B, int L, char* base) {
    Workspace w{};
    w.base = base;
    size_t o = 0;
    const size_t T = (size_t)B * L;
    auto take = [&](size_t n) { size_t at = o; o += align_up(n, 256); return base ? base + at : (char*)nullptr; };
    w.lens = (int*)take((size_t)B * 4);
    w.cu = (int*)take((size_t)(B + 1) * 4);
    w.total = (int*)take(4);
    w.order = (int*)take((size_t)B * 4);
    w.tok_src = (int*)take(T * 4);
    w.tok_pid = (int*)take(T * 4);
    w.h16 = (_Float16*)take(T * c.hidden * 2);
    w.qkv = (_Float16*)take(T * 3 * c.hidden * 2);
    w.ctx = (_Float16*)take(T * c.hidden * 2);
    w.ffn = (_Float16*)take(T * c.ffn * 2);
    w.pre = (float*)take(T * c.hidden * 4);
    w.cls16 = (_Float16*)take((size_t)B * c.hidden * 2);
    w.clspre = (float*)take((size_t)B * c.hidden * 4);
    w.h32 = c.residual_fp32 ? (float*)take(T * c.hidden * 4) : nullptr;
    w.cls32 = c.residual_fp32 ? (float*)take((size_t)B * c.hidden * 4) : nullptr;
    w.bytes = o + 256;
    return w;
}

// What every forward starts with: the workspace check (need: the caller's whole workspace, the trunk's part first), the carve behind the aligned
// base, and the packing launches -- lengths, cu_seqlens + total (+ the length order, left null in *w where attention does not walk by it) and
// token -> (source index, RoBERTa position id). The caller holds the DeviceGuard.
int trunk_begin(const Trunk& t, const long long* ids, const long long* mask, int B, int L, void* workspace_dev, size_t workspace_bytes, size_t need,
                hipStream_t st, Workspace* w) {
    if (!workspace_dev || workspace_bytes < need) return set_error(MDR_E_WORKSPACE, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    *w = carve(t.cfg, B, L, (char*)(((uintptr_t)workspace_dev + 255) & ~(uintptr_t)255));
    w->order = pack_order(w->order, B);
    launch_pack(ids, mask, B, L, t.cfg.pad_id, w->lens, w->cu, w->total, w->order, w->tok_src, w->tok_pid, st);
    return MDR_OK;
}

// The rows a layer tail runs over: every packed token, or the CLS rows of the encoder's last layer.
struct Rows {
    _Float16* h16;     // fp16 activations: the Linears' operand (and, residual_fp32 = 0, the residual)
    float* h32;        // fp32 residual stream (residual_fp32 != 0)
    float* pre;        // pre-LayerNorm sums (residual_fp32 = 2: fp16 sums in the same memory)
    int cap;           // row capacity
    const int* n_dev;  // row count on the device, or null: all cap rows are valid
    int est;           // expected rows -- tile-shape heuristics only
};

// Residual stream. residual_fp32 = 0: LayerNorm outputs live as fp16 only (GEMM operand AND residual). residual_fp32 = 1: the apex-O1 regime of
// the reference -- LayerNorm outputs stay fp32 (h32) for the residual adds, and only the copy that feeds the next Linear is rounded to fp16. In
// that mode no GEMM epilogue adds the (fp16) residual: every LayerNorm call takes it from h32 and refreshes h32 in place. residual_fp32 = 2: as 1
// with the out-projection / FFN2 outputs rounded to fp16 before the residual add (what apex O1's F.linear returns).
//
// The two Linears in front of a LayerNorm (out-projection, FFN2): r.pre = x[rows, K] W^T + bias in the mode's format. *res_in tells post_ln
// whether the GEMM already added the fp16 residual (mode 0; the large-M kernels leave it to the LayerNorm).
int gemm_to_pre(const mdr_encoder_config& c, const _Float16* x, int K, const _Float16* W, const float* bias, const Rows& r, int ncu, hipStream_t st,
                bool* res_in) {
    const int H = c.hidden;
    *res_in = true;
    if (c.residual_fp32 == 2) return launch_gemm<EPI_BIAS_F16>(x, K, W, bias, r.cap, r.n_dev, H, K, (_Float16*)r.pre, H, nullptr, 0, r.est, ncu, st);
    if (c.residual_fp32) return launch_gemm<EPI_BIAS_F32>(x, K, W, bias, r.cap, r.n_dev, H, K, r.pre, H, nullptr, 0, r.est, ncu, st);
    return launch_gemm<EPI_BIAS_RES_F32>(x, K, W, bias, r.cap, r.n_dev, H, K, r.pre, H, r.h16, H, r.est, ncu, st, res_in);
}

// r.h16 (and r.h32) = LayerNorm(r.pre + residual): the one place that knows where the residual comes from. drop (residual_fp32 = 2 only: the
// training-mode forward's callers refuse the other modes): r.pre goes through the hidden-state mask first.
void post_ln(const mdr_encoder_config& c, const Rows& r, bool res_in_gemm, const float* g, const float* b, hipStream_t st,
             const DropoutParams* drop = nullptr) {
    const bool r32 = c.residual_fp32 != 0;
    if (drop)
        launch_layernorm_dropout((const _Float16*)r.pre, (const float*)r.h32, r.cap, r.n_dev, c.hidden, g, b, c.ln_eps, *drop, r.h16, r.h32, st);
    else if (c.residual_fp32 == 2)
        launch_layernorm((const _Float16*)r.pre, (const _Float16*)nullptr, (const float*)r.h32, r.cap, r.n_dev, c.hidden, g, b, c.ln_eps, r.h16, r.h32, st);
    else
        launch_layernorm((const float*)r.pre, (const _Float16*)(r32 || res_in_gemm ? nullptr : r.h16), (const float*)(r32 ? r.h32 : nullptr), r.cap, r.n_dev,
                         c.hidden, g, b, c.ln_eps, r.h16, (float*)(r32 ? r.h32 : nullptr), st);
}

// out-projection of ctx -> LayerNorm -> FFN1 (GELU) into ffn -> FFN2 -> LayerNorm, over r. drop (with a hidden threshold): the two
// Linear outputs in front of the LayerNorms are masked at layer `li`'s ao and ff2 sites.
int layer_tail(const Trunk& t, const Layer& Ly, const _Float16* ctx, _Float16* ffn, const Rows& r, int ncu, hipStream_t st,
               const TrunkDropout* drop = nullptr, int li = 0) {
    const mdr_encoder_config& c = t.cfg;
    const int H = c.hidden, F = c.ffn;
    const bool masked = drop && drop->T_hidden;
    const DropoutParams ao = masked ? drop->params(li, kPlaceAo) : DropoutParams{}, ff2 = masked ? drop->params(li, kPlaceFf2) : DropoutParams{};
    bool res_in;
    int rc = gemm_to_pre(c, ctx, H, Ly.wo, Ly.bo, r, ncu, st, &res_in);
    if (rc) return rc;
    post_ln(c, r, res_in, Ly.ln1_g, Ly.ln1_b, st, masked ? &ao : nullptr);
    rc = launch_gemm<EPI_BIAS_GELU_F16>(r.h16, H, Ly.w1, Ly.b1, r.cap, r.n_dev, F, H, ffn, F, nullptr, 0, r.est, ncu, st);
    if (rc) return rc;
    rc = gemm_to_pre(c, ffn, F, Ly.w2, Ly.b2, r, ncu, st, &res_in);
    if (rc) return rc;
    post_ln(c, r, res_in, Ly.ln2_g, Ly.ln2_b, st, masked ? &ff2 : nullptr);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

int launch_qkv(const Trunk& t, const Layer& Ly, const Workspace& w, const Rows& r, int ncu, hipStream_t st) {
    const int H = t.cfg.hidden;
    return launch_gemm<EPI_BIAS_F16>(r.h16, H, Ly.wqkv, Ly.bqkv, r.cap, r.n_dev, 3 * H, H, w.qkv, 3 * H, nullptr, 0, r.est, ncu, st);
}

// one whole layer over every packed token (r: the token rows of w)
int trunk_layer(const Trunk& t, const Layer& Ly, const Workspace& w, const Rows& r, int B, int L, int ncu, hipStream_t st,
                const TrunkDropout* drop = nullptr, int li = 0) {
    int rc = launch_qkv(t, Ly, w, r, ncu, st);
    if (rc) return rc;
    if (drop && drop->T_attention)  // the training attention forward (include/mdr_dropout.h, mode 0): every query under the mask of layer li's attn site
        rc = mdr_attention_dropout_forward(w.qkv, w.cu, B, L, t.cfg.hidden, t.cfg.heads, 0, (int)drop->T_attention, drop->seed, drop->site(li, kPlaceAttn), w.ctx,
                                           t.device, (void*)st);
    else
        rc = launch_attention_for(MDR_ATTN_FORCE, w.qkv, w.cu, w.order, B, L, t.cfg.hidden, t.cfg.heads, w.ctx, st);
    if (rc) return rc;
    return layer_tail(t, Ly, w.ctx, w.ffn, r, ncu, st, drop, li);
}

}  // namespace
