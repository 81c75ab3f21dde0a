// csrc/mdr_reader_train.hip -- the reader's training batches assembled on the device from an item arena (include/mdr_reader_train.h).
//
// Replaces, for scripts/train_qa.py --do_train, the host work of QADataset(train=True).__getitem__ + qa_collate on every row of every batch
// of every epoch: the items are prepared once (multihop_dense_retrieval_amd/qa_train_arena.py) and a step's batch is a gather of
// `rows` of them by index. reader_train_assemble_kernel is reader_assemble_kernel's (csrc/mdr_reader_assemble.inl) shape: one 256-thread
// workgroup per row, thread t writes positions t, t + 256, ... of every output row, so each store instruction of a wave covers 64
// consecutive int64 (512 contiguous bytes); the reads are the row's int32 tokens, contiguous too. Integer copies only.
// Bounds: every arena read sits behind `valid` (0 <= index < n_items) and inside [offsets[i], offsets[i + 1]); every store is at a
// position < out_len / n_sent / n_span of row < rows.
#include "../../include/mdr_reader_train.h"
#include "mdr_common.h"

namespace mdr {
namespace {

constexpr int kTrainAssembleThreads = 256;

__global__ void __launch_bounds__(kTrainAssembleThreads)
reader_train_assemble_kernel(const int* __restrict__ a_tok, const long long* __restrict__ a_toff, const int* __restrict__ a_po,
                             const int* __restrict__ a_spos, const int* __restrict__ a_slab, const long long* __restrict__ a_sidx,
                             const int* __restrict__ a_span, const long long* __restrict__ a_pidx, const int* __restrict__ a_label,
                             const int* __restrict__ a_cov, long long n_items, const long long* __restrict__ item_idx, int Lout, int S, int P,
                             int pad_id, long long* __restrict__ o_ids, long long* __restrict__ o_mask, long long* __restrict__ o_tt,
                             long long* __restrict__ o_pm, long long* __restrict__ o_so, long long* __restrict__ o_sl, long long* __restrict__ o_st,
                             long long* __restrict__ o_en, long long* __restrict__ o_label, long long* __restrict__ o_cov,
                             long long* __restrict__ o_po, long long* __restrict__ o_len) {
    const int row = blockIdx.x, t = threadIdx.x;
    const long long it = item_idx[row];
    const bool valid = it >= 0 && it < n_items;
    long long tbeg = 0, sbeg = 0, pbeg = 0;
    int n = 0, po = 0, ns = 0, np = 0;
    if (valid) {
        tbeg = a_toff[it];
        const long long len = a_toff[it + 1] - tbeg, nsl = a_sidx[it + 1] - a_sidx[it], npl = a_pidx[it + 1] - a_pidx[it];
        n = len < 0 ? 0 : (len > 0x7fffffff ? 0x7fffffff : (int)len);
        sbeg = a_sidx[it];
        ns = nsl < 0 ? 0 : (nsl > S ? S : (int)nsl);
        pbeg = a_pidx[it];
        np = npl < 0 ? 0 : (npl > P ? P : (int)npl);
        po = a_po[it];
    }
    const int m = n < Lout ? n : Lout;  // tokens of the row that are written
    long long* ids = o_ids + (size_t)row * Lout;
    long long* msk = o_mask + (size_t)row * Lout;
    long long* tt = o_tt + (size_t)row * Lout;
    long long* pm = o_pm + (size_t)row * Lout;
    for (int p = t; p < Lout; p += kTrainAssembleThreads) {
        ids[p] = p < m ? (long long)a_tok[tbeg + p] : (long long)pad_id;
        msk[p] = p < n;
        tt[p] = p >= po && p < n;
        pm[p] = p >= po && p < n - 1;
    }
    if (o_so) {
        long long* so = o_so + (size_t)row * S;
        long long* sl = o_sl + (size_t)row * S;
        for (int j = t; j < S; j += kTrainAssembleThreads) {
            so[j] = j < ns ? (long long)a_spos[sbeg + j] : 0;
            sl[j] = j < ns ? (long long)a_slab[sbeg + j] : 0;
        }
    }
    long long* st = o_st + (size_t)row * P;
    long long* en = o_en + (size_t)row * P;
    for (int j = t; j < P; j += kTrainAssembleThreads) {
        st[j] = j < np ? (long long)a_span[2 * (pbeg + j)] : -1;
        en[j] = j < np ? (long long)a_span[2 * (pbeg + j) + 1] : -1;
    }
    if (t == 0) {
        o_label[row] = valid ? (long long)a_label[it] : -1;
        o_cov[row] = valid ? (long long)a_cov[it] : 0;
        if (o_po) o_po[row] = po;
        if (o_len) o_len[row] = n;
    }
}

}  // namespace
}  // namespace mdr

extern "C" int mdr_reader_train_assemble(const mdr_reader_train_arena* arena, const int64_t* item_idx_dev, int rows, int out_len, int n_sent,
                                         int n_span, int pad_id, const mdr_reader_train_batch* out, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_reader_train_assemble";
    MDR_REQUIRE(rows >= 0 && out_len >= 1 && n_sent >= 0 && n_span >= 1, "%s: bad shape rows=%d out_len=%d n_sent=%d n_span=%d", fn, rows, out_len,
                n_sent, n_span);
    MDR_REQUIRE(arena && out, "%s: NULL pointer", fn);
    if (rows == 0) return MDR_OK;
    MDR_REQUIRE(item_idx_dev, "%s: NULL item index", fn);
    MDR_REQUIRE(arena->n_items >= 0, "%s: n_items=%lld", fn, (long long)arena->n_items);
    MDR_REQUIRE(arena->n_items == 0 || (arena->token_offsets_dev && arena->para_offset_dev && arena->sent_index_dev && arena->span_index_dev &&
                                        arena->spans_dev && arena->label_dev && arena->ans_covered_dev),
                "%s: NULL arena array", fn);
    MDR_REQUIRE(out->input_ids && out->attention_mask && out->token_type_ids && out->paragraph_mask && out->starts && out->ends && out->label &&
                    out->ans_covered && ((out->sent_offsets && out->sent_labels) || n_sent == 0),
                "%s: NULL output pointer", fn);
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    const bool sents = n_sent > 0;
    hipLaunchKernelGGL(reader_train_assemble_kernel, dim3(rows), dim3(kTrainAssembleThreads), 0, (hipStream_t)stream, (const int*)arena->tokens_dev,
                       (const long long*)arena->token_offsets_dev, (const int*)arena->para_offset_dev, (const int*)arena->sent_pos_dev,
                       (const int*)arena->sent_label_dev, (const long long*)arena->sent_index_dev, (const int*)arena->spans_dev,
                       (const long long*)arena->span_index_dev, (const int*)arena->label_dev, (const int*)arena->ans_covered_dev,
                       (long long)arena->n_items, (const long long*)item_idx_dev, out_len, n_sent, n_span, pad_id, (long long*)out->input_ids,
                       (long long*)out->attention_mask, (long long*)out->token_type_ids, (long long*)out->paragraph_mask,
                       sents ? (long long*)out->sent_offsets : nullptr, sents ? (long long*)out->sent_labels : nullptr, (long long*)out->starts,
                       (long long*)out->ends, (long long*)out->label, (long long*)out->ans_covered, (long long*)out->para_offsets,
                       (long long*)out->lengths);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}
