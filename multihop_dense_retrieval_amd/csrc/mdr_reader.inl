// csrc/mdr_reader.inl -- the HotpotQA answer reader (QAModel at inference) on the encoder's kernels. Included at the end of
// mdr_encoder.hip, after the encoder's host code. The transformer trunk -- weight upload, workspace, packing and every layer -- is the
// shared one of mdr_encoder_trunk.inl; this file adds the reader's own embedding kernel, its pooler and heads, and the span search.
// Not a translation unit of its own.
//
// Replaces
//   /root/reference/mdr/qa/qa_model.py:50-81        encoder(ids, mask, token_type_ids) -> qa_outputs / pooler + rank / sp heads
//   /root/reference/scripts/train_qa.py:233-253      sp mask + sigmoid, the band-limited [B, L, L] span matrix and its two-stage max
// where `encoder` is HF ElectraModel (or BertModel). Kernels
//   reader_embed_ln      word + absolute position (0-based within the row) + token_type[type_id], LayerNorm -> fp16 (+ fp32 stream)
//   reader_logits        start / end logits per position: a 2 x H dot on the final hidden state, -inf outside paragraph_mask
//   reader_rank          tanh of the pooler dense output (the dense itself is an encoder GEMM on the CLS rows), then the rank dot
//   reader_sp            sp logit at each sent_offsets entry, the sent_offsets == 0 -> -inf mask and the sigmoid
//   reader_span          per sequence: max over s <= e <= s + max_ans_len of start[s] + end[e] without the [L, L] matrix
//
// Rounding points of the heads (apex O1, the README's --fp16 regime):
//   - every head Linear casts its weight AND bias to fp16 and returns fp16 (F.linear is an fp16 function under O1): the dots here
//     accumulate fp32 products of fp16 operands, add the fp16-rounded bias and round once to fp16;
//   - the input of the heads is the fp16 copy of the last LayerNorm's output (that LayerNorm runs in fp32; the Linear casts it);
//   - tanh (pooler) and sigmoid (sp) take an fp16 tensor: computed in fp32, rounded to fp16;
//   - masked_fill(-inf) on fp16 values stays -inf; the span matrix's out-of-band fill -1e10 rounds to -inf under .type_as(fp16);
//   - start + end is an fp16 add (the exact fp32 sum of two fp16 values rounded to fp16), so exact ties are common and the
//     tie rule decides: torch's max returns the first index, over e first and then over s, i.e. the row-major-first (s, e).

namespace mdr {
namespace {

__device__ inline float h16_bits_to_f(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
__device__ inline unsigned short f_to_h16_bits(float x) { return __builtin_bit_cast(unsigned short, (_Float16)x); }
constexpr unsigned short kH16NegInf = 0xFC00u;

// one wave per packed token (the layout of embed_ln_kernel); positions are absolute within the row (BERT / ELECTRA), not the
// RoBERTa padding-offset ids the encoder computes, so the row position comes from the token's source index.
__global__ void __launch_bounds__(256)
reader_embed_ln_kernel(const long long* __restrict__ ids, const long long* __restrict__ types, const int* __restrict__ tok_src,
                       const int* __restrict__ total, int L, const float* __restrict__ word, const float* __restrict__ pos,
                       const float* __restrict__ type_emb, int type_vocab, const float* __restrict__ g, const float* __restrict__ bta, int H,
                       int vocab, float eps, _Float16* __restrict__ out, float* __restrict__ out32) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= *total) return;
    const int src = tok_src[t];
    const int p = src % L;  // < L <= max_pos (checked on the host)
    long long id = ids[src];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    long long ty = types ? types[src] : 0;
    ty = ty < 0 ? 0 : (ty >= type_vocab ? type_vocab - 1 : ty);
    const float* wr = word + (size_t)id * H;
    const float* pr = pos + (size_t)p * H;
    const float* tr = type_emb + (size_t)ty * H;
    const int n = H >> 6;
    float x[kMaxPerLane];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kMaxPerLane; ++i)
        if (i < n) { int e = lane + 64 * i; x[i] = wr[e] + pr[e] + tr[e]; s += x[i]; }
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
            out[(size_t)t * H + e] = (_Float16)y;
            if (out32) out32[(size_t)t * H + e] = y;
        }
}

// fp32 dot of an fp16 row with an fp16 weight row over one wave (H % 128 == 0: one half2 per lane per step)
__device__ inline float wave_dot_h16(const _Float16* __restrict__ x, const _Float16* __restrict__ w, int H) {
    typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63;
    float acc = 0.f;
    for (int e = 2 * lane; e < H; e += 128) {
        const half2_t a = *(const half2_t*)(x + e), b = *(const half2_t*)(w + e);
        acc += (float)a[0] * (float)b[0] + (float)a[1] * (float)b[1];
    }
    return wave_sum(acc);
}

// one wave per (b, p) of the padded [B, L] output; the packed token of a right-padded row is cu[b] + p
__global__ void __launch_bounds__(256)
reader_logits_kernel(const _Float16* __restrict__ h, const int* __restrict__ cu, const long long* __restrict__ pmask, int B, int L, int H,
                     const _Float16* __restrict__ w2, const float* __restrict__ b2, unsigned short* __restrict__ start_out,
                     unsigned short* __restrict__ end_out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B * L) return;
    const int b = i / L, p = i - b * L;
    const int len = cu[b + 1] - cu[b];
    if (p >= len || pmask[i] != 1) {
        if (lane == 0) { start_out[i] = kH16NegInf; end_out[i] = kH16NegInf; }
        return;
    }
    const _Float16* x = h + (size_t)(cu[b] + p) * H;
    const float s = wave_dot_h16(x, w2, H) + b2[0];
    const float e = wave_dot_h16(x, w2 + H, H) + b2[1];
    if (lane == 0) { start_out[i] = f_to_h16_bits(s); end_out[i] = f_to_h16_bits(e); }
}

// one wave per sequence: pooled = fp16(tanh(fp16 dense output)); rank = fp16(pooled . w + b)
__global__ void __launch_bounds__(256)
reader_rank_kernel(const _Float16* __restrict__ dense, int B, int H, const _Float16* __restrict__ w, const float* __restrict__ bias,
                   unsigned short* __restrict__ rank_out) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float acc = 0.f;
    for (int e = lane; e < H; e += 64) {
        const _Float16 pooled = (_Float16)tanhf((float)dense[(size_t)b * H + e]);
        acc += (float)pooled * (float)w[e];
    }
    acc = wave_sum(acc);
    if (lane == 0) rank_out[b] = f_to_h16_bits(acc + bias[0]);
}

// one wave per (b, j): the sp Linear on the hidden state at sent_offsets[b, j] (QAModel's torch.gather), then predict()'s
// masked_fill(sent_offsets == 0, -inf) and sigmoid, both on fp16 values
__global__ void __launch_bounds__(256)
reader_sp_kernel(const _Float16* __restrict__ h, const int* __restrict__ cu, const long long* __restrict__ offs, int B, int L, int NS, int H,
                 const _Float16* __restrict__ w, const float* __restrict__ bias, unsigned short* __restrict__ score_out,
                 unsigned short* __restrict__ prob_out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B * NS) return;
    const int b = i / NS;
    const long long p = offs[i];
    const int len = cu[b + 1] - cu[b];
    unsigned short sc = kH16NegInf;
    if (p >= 0 && p < len) sc = f_to_h16_bits(wave_dot_h16(h + (size_t)(cu[b] + (int)p) * H, w, H) + bias[0]);
    if (lane == 0) {
        if (score_out) score_out[i] = sc;
        if (prob_out) {
            const float x = p == 0 ? -INFINITY : h16_bits_to_f(sc);
            prob_out[i] = f_to_h16_bits(1.f / (1.f + expf(-x)));
        }
    }
}

// (score, s, e) ordered by score, then row-major position: "a beats b" is torch's first-index max over e, then over s
struct SpanBest { float v; int s, e; };
__device__ inline bool span_beats(const SpanBest& a, const SpanBest& b) {
    return a.v > b.v || (a.v == b.v && (a.s < b.s || (a.s == b.s && a.e < b.e)));
}

// one workgroup of 256 per sequence; start / end of the row in LDS; thread t walks the rows s = t, t + 256, ... and for each the
// band e in [s, min(s + max_ans_len, L - 1)], then the workgroup reduces. Every in-band sum is an fp16 add; out-of-band cells
// are -inf (the -1e10 fill under fp16) and are never better than the in-band cell (0, 0), so the walk over the band alone is exact.
constexpr int kSpanMaxL = 512;
__global__ void __launch_bounds__(256)
reader_span_kernel(const unsigned short* __restrict__ start, const unsigned short* __restrict__ end, int L, int max_ans_len,
                   long long* __restrict__ s_out, long long* __restrict__ e_out, unsigned short* __restrict__ score_out) {
    __shared__ float st[kSpanMaxL], en[kSpanMaxL];
    __shared__ SpanBest wbest[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int p = tid; p < L; p += 256) {
        st[p] = h16_bits_to_f(start[(size_t)b * L + p]);
        en[p] = h16_bits_to_f(end[(size_t)b * L + p]);
    }
    __syncthreads();
    SpanBest best{-INFINITY, 0x7fffffff, 0x7fffffff};
    for (int s = tid; s < L; s += 256) {
        const int e_hi = (int)min((long long)L - 1, (long long)s + max_ans_len);
        const float a = st[s];
        for (int e = s; e <= e_hi; ++e) {
            const float v = (float)(_Float16)(a + en[e]);
            // rows are walked in increasing s by this thread and e increases inside a row: a later cell wins only if strictly greater
            // (or if it is the first cell seen: the -inf row of a fully masked band still has to give its (s, e))
            if (v > best.v || best.s == 0x7fffffff) best = SpanBest{v, s, e};
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        SpanBest other{__shfl_xor(best.v, o), __shfl_xor(best.s, o), __shfl_xor(best.e, o)};
        if (span_beats(other, best)) best = other;
    }
    if (lane == 0) wbest[w] = best;
    __syncthreads();
    if (tid == 0) {
        best = wbest[0];
        for (int i = 1; i < 4; ++i)
            if (span_beats(wbest[i], best)) best = wbest[i];
        s_out[b] = best.s;
        e_out[b] = best.e;
        score_out[b] = f_to_h16_bits(best.v);
    }
}

__global__ void h16_round_f32_kernel(float* __restrict__ x, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = (float)(_Float16)x[i];
}

}  // namespace
}  // namespace mdr

struct mdr_reader {
    mdr_reader_config cfg{};
    Trunk t;                    // t.type: the whole [type_vocab, H] table
    _Float16* wpool = nullptr;  // pooler dense [H, H]
    float* bpool = nullptr;
    _Float16* whead = nullptr;  // [4, H] rows: start, end, rank, sp
    float* bhead = nullptr;     // [4], fp16-rounded (apex O1 casts the bias with the weight)
};

namespace {

mdr_encoder_config reader_trunk_config(const mdr_reader_config& c) {
    mdr_encoder_config e{};
    e.vocab = c.vocab; e.hidden = c.hidden; e.layers = c.layers; e.heads = c.heads; e.ffn = c.ffn; e.max_pos = c.max_pos;
    e.pad_id = 0; e.ln_eps = c.ln_eps; e.residual_fp32 = c.residual_fp32;
    return e;
}

// behind the trunk's workspace: the logits, when the caller does not keep them but the span search needs them
struct ReaderWs {
    unsigned short *start16, *end16;
    size_t bytes;
};

ReaderWs reader_carve(const Workspace& enc, int B, int L) {
    ReaderWs r{};
    size_t o = align_up(enc.bytes, 256);
    auto take = [&](size_t n) { size_t at = o; o += align_up(n, 256); return enc.base ? enc.base + at : (char*)nullptr; };
    r.start16 = (unsigned short*)take((size_t)B * L * 2);
    r.end16 = (unsigned short*)take((size_t)B * L * 2);
    r.bytes = o + 256;
    return r;
}

int launch_span_search(const unsigned short* start, const unsigned short* end, int B, int L, int max_ans_len, long long* s_out, long long* e_out,
                       unsigned short* score_out, hipStream_t st) {
    hipLaunchKernelGGL(reader_span_kernel, dim3(B), dim3(256), 0, st, start, end, L, max_ans_len, s_out, e_out, score_out);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

// the reader's embedding launch (position = source index % L, a type table; types may be null): one wave per packed token, cap = batch * seq_len
void launch_reader_embed_ln(const long long* ids, const long long* types, const int* tok_src, const int* total, int cap, int L, const float* word,
                            const float* pos, const float* type_emb, int type_vocab, const float* g, const float* b, int H, int vocab, float eps,
                            _Float16* out16, float* out32, hipStream_t st) {
    hipLaunchKernelGGL(reader_embed_ln_kernel, dim3((cap + 3) / 4), dim3(256), 0, st, ids, types, tok_src, total, L, word, pos, type_emb, type_vocab, g, b, H,
                       vocab, eps, out16, out32);
}

}  // namespace

extern "C" {

int mdr_reader_create(const mdr_reader_config* cfg, const mdr_tensor* tensors, int n_tensors, int weights_on_device, int device, void* stream,
                      mdr_reader** out) {
    MDR_REQUIRE(cfg && tensors && out, "NULL argument");
    MDR_REQUIRE(cfg->type_vocab > 0, "bad geometry");
    MDR_REQUIRE(cfg->pooler == MDR_READER_POOLER_HEAD || cfg->pooler == MDR_READER_POOLER_ENCODER, "pooler=%d unknown", cfg->pooler);
    for (int i = 0; i < n_tensors; ++i)
        MDR_REQUIRE(!(tensors[i].name && std::strncmp(tensors[i].name, "encoder.embeddings_project.", 27) == 0),
                    "embeddings_project (embedding size != hidden, ELECTRA-small) is not supported");
    const mdr_encoder_config tc = reader_trunk_config(*cfg);
    if (int rc = trunk_check(tc, device)) return rc;
    DeviceGuard guard(device);
    hipStream_t st = (hipStream_t)stream;
    mdr_reader* h = new (std::nothrow) mdr_reader();
    MDR_REQUIRE(h != nullptr, "out of host memory");
    h->cfg = *cfg;
    const size_t H = cfg->hidden;
    WeightLoader ld{tensors, n_tensors, weights_on_device, st, &h->t.allocs};
    trunk_upload(h->t, tc, device, cfg->type_vocab, ld);
    const std::string PL = cfg->pooler == MDR_READER_POOLER_HEAD ? "pooler.dense." : "encoder.pooler.dense.";
    ld.keep16(PL + "weight", H * H, &h->wpool);
    ld.keep32(PL + "bias", H, &h->bpool);
    // the four head rows go through the fp32 staging buffer in one [4, H] block (the sp row stays 0 without sp.*)
    ld.alloc(4 * H * 2, (void**)&h->whead);
    ld.alloc(4 * 4, (void**)&h->bhead);
    if (!ld.rc && (hipMemsetAsync(ld.staging, 0, 4 * H * 4, st) != hipSuccess || hipMemsetAsync(h->bhead, 0, 16, st) != hipSuccess))
        ld.rc = set_error(MDR_E_HIP, "hipMemsetAsync failed");
    ld.fetch32("qa_outputs.weight", 2 * H, ld.staging);
    ld.fetch32("qa_outputs.bias", 2, h->bhead);
    ld.fetch32("rank.weight", H, ld.staging, 2 * H);
    ld.fetch32("rank.bias", 1, h->bhead, 2);
    if (cfg->has_sp) {
        ld.fetch32("sp.weight", H, ld.staging, 3 * H);
        ld.fetch32("sp.bias", 1, h->bhead, 3);
    }
    ld.convert16(4 * H, h->whead);
    if (!ld.rc) {
        hipLaunchKernelGGL(h16_round_f32_kernel, dim3(1), dim3(64), 0, st, h->bhead, 4);
        if (hipGetLastError() != hipSuccess) ld.rc = set_error(MDR_E_HIP, "head weight conversion failed");
    }
    if (int rc = ld.finish()) {
        mdr_reader_free(h);
        return rc;
    }
    *out = h;
    return MDR_OK;
}

int mdr_reader_free(mdr_reader* h) {
    if (!h) return MDR_OK;
    trunk_free(h->t);
    delete h;
    return MDR_OK;
}

size_t mdr_reader_workspace_bytes(const mdr_reader* h, int batch, int seq_len, int n_sent) {
    (void)n_sent;
    if (!h || batch <= 0 || seq_len <= 0) return 0;
    return reader_carve(carve(h->t.cfg, batch, seq_len, nullptr), batch, seq_len).bytes;
}

int mdr_reader_span_search(const uint16_t* start_logits_dev, const uint16_t* end_logits_dev, int batch, int seq_len, int max_ans_len,
                           int64_t* span_start_dev, int64_t* span_end_dev, uint16_t* span_score_dev, int device, void* stream) {
    MDR_REQUIRE(batch >= 0 && seq_len > 0 && seq_len <= kSpanMaxL, "bad shape batch=%d seq_len=%d (seq_len <= %d)", batch, seq_len, kSpanMaxL);
    MDR_REQUIRE(max_ans_len >= 0, "max_ans_len=%d must be >= 0", max_ans_len);
    if (batch == 0) return MDR_OK;
    MDR_REQUIRE(start_logits_dev && end_logits_dev && span_start_dev && span_end_dev && span_score_dev, "NULL pointer");
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    return launch_span_search(start_logits_dev, end_logits_dev, batch, seq_len, max_ans_len, (long long*)span_start_dev, (long long*)span_end_dev,
                              span_score_dev, (hipStream_t)stream);
}

int mdr_reader_forward(mdr_reader* h, const int64_t* ids_dev, const int64_t* mask_dev, const int64_t* token_type_ids_dev,
                       const int64_t* paragraph_mask_dev, const int64_t* sent_offsets_dev, int batch, int seq_len, int n_sent, int max_ans_len,
                       const mdr_reader_outputs* o, void* workspace_dev, size_t workspace_bytes, void* stream) {
    MDR_REQUIRE(h != nullptr && o != nullptr, "reader handle or outputs is NULL");
    MDR_REQUIRE(batch >= 0 && seq_len > 0 && n_sent >= 0, "bad shape batch=%d seq_len=%d n_sent=%d", batch, seq_len, n_sent);
    if (batch == 0) return MDR_OK;
    const mdr_reader_config& rc_ = h->cfg;
    MDR_REQUIRE(seq_len <= kSpanMaxL && seq_len <= rc_.max_pos, "seq_len=%d exceeds min(%d, max_pos=%d)", seq_len, kSpanMaxL, rc_.max_pos);
    MDR_REQUIRE((long long)batch * seq_len < (1ll << 31), "batch*seq_len overflows int32; split the batch");
    MDR_REQUIRE(ids_dev && mask_dev && paragraph_mask_dev, "NULL input pointer");
    MDR_REQUIRE(n_sent == 0 || sent_offsets_dev, "sent_offsets is NULL with n_sent=%d", n_sent);
    MDR_REQUIRE(!(o->sp_score || o->sp_prob) || rc_.has_sp, "sp outputs requested but the reader has no sp head (has_sp=0)");
    MDR_REQUIRE(max_ans_len >= 0 || !o->span_start, "max_ans_len=%d must be >= 0", max_ans_len);
    MDR_REQUIRE(!o->span_start || (o->span_end && o->span_score), "span_start given without span_end / span_score");
    const Trunk& t = h->t;
    const mdr_encoder_config& c = t.cfg;
    DeviceGuard guard(t.device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", t.device);
    hipStream_t st = (hipStream_t)stream;
    const long long* ids = (const long long*)ids_dev;
    const size_t need = reader_carve(carve(c, batch, seq_len, nullptr), batch, seq_len).bytes;
    Workspace w;  // packing as in the encoder (tok_pid, the RoBERTa position ids, is not read here)
    if (int rc = trunk_begin(t, ids, (const long long*)mask_dev, batch, seq_len, workspace_dev, workspace_bytes, need, st, &w)) return rc;
    const ReaderWs rw = reader_carve(w, batch, seq_len);
    const int B = batch, L = seq_len, H = c.hidden, ncu = t.num_cus;
    const int Tcap = B * L;
    launch_reader_embed_ln(ids, (const long long*)token_type_ids_dev, w.tok_src, w.total, Tcap, L, t.word, t.pos, t.type, rc_.type_vocab, t.emb_g, t.emb_b, H,
                           c.vocab, c.ln_eps, w.h16, w.h32, st);
    MDR_HIP_TRY(hipGetLastError());
    // every layer over all packed tokens: the heads need every token's final hidden state
    const Rows tokens{w.h16, w.h32, w.pre, Tcap, w.total, Tcap - Tcap / 3};
    int rc;
    for (const Layer& Ly : t.layers) {
        rc = trunk_layer(t, Ly, w, tokens, B, L, ncu, st);
        if (rc) return rc;
    }
    // ---- heads on the fp16 final hidden states w.h16 [T, H] ----
    unsigned short* start16 = o->start_logits ? o->start_logits : rw.start16;
    unsigned short* end16 = o->end_logits ? o->end_logits : rw.end16;
    if (o->start_logits || o->end_logits || o->span_start)
        hipLaunchKernelGGL(reader_logits_kernel, dim3((Tcap + 3) / 4), dim3(256), 0, st, (const _Float16*)w.h16, (const int*)w.cu,
                           (const long long*)paragraph_mask_dev, B, L, H, (const _Float16*)h->whead, (const float*)h->bhead, start16, end16);
    if (o->rank_score) {
        _Float16* dense16 = (_Float16*)w.clspre;  // pooler dense output [B, H] fp16 (apex O1: the Linear returns fp16)
        launch_gather_cls(w.h16, (const float*)nullptr, w.cu, B, H, w.cls16, (float*)nullptr, st);
        rc = launch_gemm<EPI_BIAS_F16>(w.cls16, H, h->wpool, h->bpool, B, nullptr, H, H, dense16, H, nullptr, 0, B, ncu, st);
        if (rc) return rc;
        hipLaunchKernelGGL(reader_rank_kernel, dim3((B + 3) / 4), dim3(256), 0, st, (const _Float16*)dense16, B, H,
                           (const _Float16*)(h->whead + (size_t)2 * H), (const float*)(h->bhead + 2), o->rank_score);
    }
    if ((o->sp_score || o->sp_prob) && n_sent > 0)
        hipLaunchKernelGGL(reader_sp_kernel, dim3((B * n_sent + 3) / 4), dim3(256), 0, st, (const _Float16*)w.h16, (const int*)w.cu,
                           (const long long*)sent_offsets_dev, B, L, n_sent, H, (const _Float16*)(h->whead + (size_t)3 * H), (const float*)(h->bhead + 3),
                           o->sp_score, o->sp_prob);
    MDR_HIP_TRY(hipGetLastError());
    if (o->span_start) {
        rc = launch_span_search(start16, end16, B, L, max_ans_len, (long long*)o->span_start, (long long*)o->span_end, o->span_score, st);
        if (rc) return rc;
    }
    return MDR_OK;
}

}  // extern "C"

// the training loss and the heads with gradients (include/mdr_reader_loss.h): the heads' forward is the three kernels above
#include "mdr_reader_loss.inl"
