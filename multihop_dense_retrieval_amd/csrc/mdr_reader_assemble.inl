// csrc/mdr_reader_assemble.inl -- device-side construction of the reader's input rows from a QA passage arena (included from
// mdr_encoder.hip after mdr_reader.inl).
//
// Replaces, for the end-to-end path, the host work of mdr/qa/qa_dataset.py QAEvalDataset.__getitem__ + qa_collate on every chain:
// prepare() splits "yes no [SEP] " + " [SEP] ".join(passage strings) on whitespace and WordPiece-tokenises word by word, so a chain's
// WordPiece sequence is yes no [SEP] P1 [SEP] P2 where each Pi depends on passage i alone. The corpus is tokenised once into an arena
// (multihop_dense_retrieval_amd/qa_arena.py); this kernel splices the rows, as assemble_hop2_kernel does for the retriever's hop 2.

namespace mdr {
namespace {

struct ReaderSpecial {
    int cls, sep, yes, no, pad;
};

// one 256-thread workgroup per chain row
__global__ void __launch_bounds__(256)
reader_assemble_kernel(const long long* __restrict__ q_ids, const long long* __restrict__ q_lens, int n_q, int q_stride,
                       const long long* __restrict__ chains, const long long* __restrict__ row_q, const int* __restrict__ a_tok,
                       const long long* __restrict__ a_toff, const int* __restrict__ a_ss, const long long* __restrict__ a_soff, long long n_pass,
                       ReaderSpecial sp, int max_seq_len, int Lout, int S, long long* __restrict__ o_ids, long long* __restrict__ o_mask,
                       long long* __restrict__ o_tt, long long* __restrict__ o_pm, long long* __restrict__ o_so, long long* __restrict__ o_po,
                       long long* __restrict__ o_len) {
    const int row = blockIdx.x, t = threadIdx.x;
    const long long b = row_q[row];
    const bool has_q = b >= 0 && b < n_q;
    int ql = 0;
    if (has_q) {
        const long long v = q_lens[b];
        ql = v < 0 ? 0 : (v > q_stride ? q_stride : (int)v);
    }
    const long long* qrow = q_ids + (size_t)(has_q ? b : 0) * q_stride;
    long long beg0 = 0, beg1 = 0, sbeg0 = 0, sbeg1 = 0;
    int len0 = 0, len1 = 0, ns0 = 0, ns1 = 0;
    const long long c0 = chains[(size_t)row * 2], c1 = chains[(size_t)row * 2 + 1];
    if (c0 >= 0 && c0 < n_pass) {
        beg0 = a_toff[c0];
        len0 = (int)(a_toff[c0 + 1] - beg0);
        sbeg0 = a_soff[c0];
        ns0 = (int)(a_soff[c0 + 1] - sbeg0);
    }
    if (c1 >= 0 && c1 < n_pass) {
        beg1 = a_toff[c1];
        len1 = (int)(a_toff[c1 + 1] - beg1);
        sbeg1 = a_soff[c1];
        ns1 = (int)(a_soff[c1 + 1] - sbeg1);
    }
    const int po = ql + 2;               // para_offset
    const int wp = 3 + len0 + 1 + len1;  // yes no [SEP] P1 [SEP] P2
    int cut = max_seq_len - po - 1;
    cut = cut < 0 ? 0 : (wp < cut ? wp : cut);
    const int n = po + cut + 1;
    const int p2 = 4 + len0;  // wp position of P2's first token
    long long* ids = o_ids + (size_t)row * Lout;
    long long* msk = o_mask + (size_t)row * Lout;
    long long* tt = o_tt + (size_t)row * Lout;
    long long* pm = o_pm + (size_t)row * Lout;
    for (int p = t; p < Lout; p += 256) {
        long long v = sp.pad;
        if (p == 0) {
            v = sp.cls;
        } else if (p <= ql) {
            v = qrow[p - 1];
        } else if (p == ql + 1) {
            v = sp.sep;
        } else if (p < po + cut) {
            const int w = p - po;
            if (w == 0) v = sp.yes;
            else if (w == 1) v = sp.no;
            else if (w == 2 || w == p2 - 1) v = sp.sep;
            else if (w < p2 - 1) v = a_tok[beg0 + (w - 3)];
            else v = a_tok[beg1 + (w - p2)];
        } else if (p == po + cut) {
            v = sp.sep;
        }
        ids[p] = v;
        msk[p] = p < n;
        tt[p] = p >= po && p < n;
        pm[p] = p >= po && p < n - 1;
    }
    if (o_so) {
        long long* so = o_so + (size_t)row * S;
        for (int j = t; j < S; j += 256) {
            long long v = 0;
            if (j < ns0) {
                const int w = 3 + a_ss[sbeg0 + j];
                if (w < cut) v = w + po;
            } else if (j < ns0 + ns1) {
                const int w = p2 + a_ss[sbeg1 + (j - ns0)];
                if (w < cut) v = w + po;
            }
            so[j] = v;
        }
    }
    if (t == 0) {
        if (o_po) o_po[row] = po;
        if (o_len) o_len[row] = n;
    }
}

}  // namespace
}  // namespace mdr

extern "C" int mdr_reader_assemble(const int64_t* q_ids_dev, const int64_t* q_lens_dev, int n_questions, int q_stride, const int64_t* chains_dev,
                                   const int64_t* row_question_dev, int rows, const mdr_reader_arena* arena, const int32_t* special, int max_seq_len,
                                   int out_len, int n_sent, const mdr_reader_batch* out, int device, void* stream) {
    using namespace mdr;
    MDR_REQUIRE(rows >= 0 && n_questions >= 0 && q_stride >= 0 && out_len >= 1 && n_sent >= 0,
                "bad shape rows=%d n_questions=%d q_stride=%d out_len=%d n_sent=%d", rows, n_questions, q_stride, out_len, n_sent);
    MDR_REQUIRE(max_seq_len - q_stride >= 6, "max_seq_len=%d leaves no room for yes no [SEP] after a question of %d tokens", max_seq_len, q_stride);
    MDR_REQUIRE(arena && special && out, "NULL pointer");
    if (rows == 0) return MDR_OK;
    MDR_REQUIRE(q_lens_dev && chains_dev && row_question_dev && (q_ids_dev || q_stride == 0), "NULL input pointer");
    MDR_REQUIRE(arena->n_passages >= 0 && arena->token_offsets_dev && arena->sent_offsets_dev, "NULL arena offsets");
    MDR_REQUIRE(out->input_ids && out->attention_mask && out->token_type_ids && out->paragraph_mask && (out->sent_offsets || n_sent == 0),
                "NULL output pointer");
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    ReaderSpecial sp{special[0], special[1], special[2], special[3], special[4]};
    hipLaunchKernelGGL(reader_assemble_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, (const long long*)q_ids_dev, (const long long*)q_lens_dev,
                       n_questions, q_stride, (const long long*)chains_dev, (const long long*)row_question_dev, (const int*)arena->tokens_dev,
                       (const long long*)arena->token_offsets_dev, (const int*)arena->sent_starts_dev, (const long long*)arena->sent_offsets_dev,
                       (long long)arena->n_passages, sp, max_seq_len, out_len, n_sent, (long long*)out->input_ids, (long long*)out->attention_mask,
                       (long long*)out->token_type_ids, (long long*)out->paragraph_mask, n_sent ? (long long*)out->sent_offsets : nullptr,
                       (long long*)out->para_offsets, (long long*)out->lengths);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}
