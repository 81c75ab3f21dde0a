// csrc/mdr_reader_train_pieces.hip -- the reader's training batches spliced on the device from a PIECE arena
// (include/mdr_reader_train_pieces.h): what mdr_reader_train_assemble (csrc/mdr_reader_train.hip) gathers from finished rows, built here
// from one stored row per question and per distinct passage, so that the 100 candidate chains of a question do not store (nor, when the
// run starts, tokenise) the question and their shared passages 100 times (multihop_dense_retrieval_amd/qa_train_pieces.py).
//
// reader_train_compose_kernel is reader_assemble_kernel's (csrc/mdr_reader_assemble.inl) shape: one 256-thread workgroup per row, thread t
// writes positions t, t + 256, ... of every output row, so each store instruction of a wave covers 64 consecutive int64 (512 contiguous
// bytes); the reads are int32 runs of the question and of the two passages, contiguous too. Integer copies only. The spans that start
// inside the cut are compacted in stored order by a ballot per wave and four wave counts in LDS: no atomics, one order.
// Bounds: every arena read sits behind `valid` (0 <= index < n_items); the rows it names lie inside their tables and every index array is
// monotone (checked once on the host by the caller); token reads are at positions < cut <= 4 + len0 + len1, sentence reads at ordinals
// < ns0 + ns1, label reads only where the item holds ns0 + ns1 of them, pair reads at < the item's pair count; every store is at a
// position < out_len / n_sent / n_span of row < rows.
#include "../../include/mdr_reader_train_pieces.h"
#include "mdr_common.h"

namespace mdr {
namespace {

constexpr int kComposeThreads = 256;
constexpr int kComposeWaves = kComposeThreads / 64;

struct ComposeSpecial {
    int cls, sep, yes, no, pad;
};

__device__ __forceinline__ int clamp_count(long long v) { return v < 0 ? 0 : (v > 0x7fffffff ? 0x7fffffff : (int)v); }

__global__ void __launch_bounds__(kComposeThreads)
reader_train_compose_kernel(mdr_reader_train_pieces a, const long long* __restrict__ item_idx, ComposeSpecial sp, int max_seq_len, int Lout, int S,
                            int P, mdr_reader_train_batch o) {
    __shared__ int wave_kept[kComposeWaves];
    const int row = blockIdx.x, t = threadIdx.x;
    const long long it = item_idx[row];
    const bool valid = it >= 0 && it < a.n_items;
    long long qbeg = 0, beg0 = 0, beg1 = 0, sbeg0 = 0, sbeg1 = 0, lbeg = 0, pbeg = 0;
    int ql = 0, len0 = 0, len1 = 0, ns0 = 0, ns1 = 0, nl = 0, np = 0, label = -1, cov = 0;
    if (valid) {
        const int* rec = a.items_dev + it * 5;
        const long long q = rec[0], c0 = rec[1], c1 = rec[2];
        label = rec[3];
        cov = rec[4];
        qbeg = a.q_offsets_dev[q];
        ql = clamp_count(a.q_offsets_dev[q + 1] - qbeg);
        beg0 = a.p_offsets_dev[c0];
        len0 = clamp_count(a.p_offsets_dev[c0 + 1] - beg0);
        sbeg0 = a.p_sent_offsets_dev[c0];
        ns0 = clamp_count(a.p_sent_offsets_dev[c0 + 1] - sbeg0);
        beg1 = a.p_offsets_dev[c1];
        len1 = clamp_count(a.p_offsets_dev[c1 + 1] - beg1);
        sbeg1 = a.p_sent_offsets_dev[c1];
        ns1 = clamp_count(a.p_sent_offsets_dev[c1 + 1] - sbeg1);
        lbeg = a.sent_label_index_dev[it];
        nl = clamp_count(a.sent_label_index_dev[it + 1] - lbeg);
        pbeg = a.span_index_dev[it];
        np = clamp_count(a.span_index_dev[it + 1] - pbeg);
    }
    const int po = valid ? ql + 2 : 0;   // para_offset
    const int wp = 3 + len0 + 1 + len1;  // yes no [SEP] P1 [SEP] P2
    int cut = max_seq_len - po - 1;
    cut = !valid || cut < 0 ? 0 : (wp < cut ? wp : cut);
    const int n = valid ? po + cut + 1 : 0;
    const int p2 = 4 + len0;  // wp position of P2's first token
    int64_t* ids = o.input_ids + (size_t)row * Lout;
    int64_t* msk = o.attention_mask + (size_t)row * Lout;
    int64_t* tt = o.token_type_ids + (size_t)row * Lout;
    int64_t* pm = o.paragraph_mask + (size_t)row * Lout;
    for (int p = t; p < Lout; p += kComposeThreads) {
        long long v = sp.pad;
        if (p < n) {
            if (p == 0) {
                v = sp.cls;
            } else if (p <= ql) {
                v = a.q_tokens_dev[qbeg + (p - 1)];
            } else if (p == ql + 1 || p == po + cut) {
                v = sp.sep;
            } else {
                const int w = p - po;
                if (w == 0) v = sp.yes;
                else if (w == 1) v = sp.no;
                else if (w == 2 || w == p2 - 1) v = sp.sep;
                else if (w < p2 - 1) v = a.p_tokens_dev[beg0 + (w - 3)];
                else v = a.p_tokens_dev[beg1 + (w - p2)];
            }
        }
        ids[p] = v;
        msk[p] = p < n;
        tt[p] = p >= po && p < n;
        pm[p] = p >= po && p < n - 1;
    }
    if (o.sent_offsets) {
        int64_t* so = o.sent_offsets + (size_t)row * S;
        int64_t* sl = o.sent_labels + (size_t)row * S;
        const bool labelled = nl == ns0 + ns1;  // an item holds one label per sentence of its chain, or none
        for (int j = t; j < S; j += kComposeThreads) {
            long long off = 0, lab = 0;
            if (j < ns0 + ns1) {  // the starts increase along the chain: those inside the cut are a prefix of the ordinals
                const int w = j < ns0 ? 3 + a.p_sent_starts_dev[sbeg0 + j] : p2 + a.p_sent_starts_dev[sbeg1 + (j - ns0)];
                if (w < cut) {
                    off = w + po;
                    if (labelled) lab = a.sent_label_dev[lbeg + j];
                }
            }
            so[j] = off;
            sl[j] = lab;
        }
    }
    // spans: pair i is kept when its first position lies inside the cut; kept pairs keep their stored order
    int64_t* st = o.starts + (size_t)row * P;
    int64_t* en = o.ends + (size_t)row * P;
    const int lane = t & 63, wave = t >> 6;
    int kept = 0;  // uniform over the workgroup
    for (int base = 0; base < np && kept < P; base += kComposeThreads) {
        const int i = base + t;
        int first = 0, last = 0;
        bool keep = false;
        if (i < np) {
            first = a.spans_dev[2 * (pbeg + i)];
            last = a.spans_dev[2 * (pbeg + i) + 1];
            keep = first < cut;
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(mask);
        __syncthreads();
        int slot = kept + __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < kComposeWaves; ++w) {
            if (w < wave) slot += wave_kept[w];
            total += wave_kept[w];
        }
        if (keep && slot < P) {
            st[slot] = first + po;
            en[slot] = (last < cut - 1 ? last : cut - 1) + po;
        }
        kept += total;
        __syncthreads();  // wave_kept is rewritten by the next round
    }
    for (int j = (kept < P ? kept : P) + t; j < P; j += kComposeThreads) {
        st[j] = -1;
        en[j] = -1;
    }
    if (t == 0) {
        o.label[row] = label;
        o.ans_covered[row] = cov;
        if (o.para_offsets) o.para_offsets[row] = po;
        if (o.lengths) o.lengths[row] = n;
    }
}

}  // namespace
}  // namespace mdr

extern "C" int mdr_reader_train_compose(const mdr_reader_train_pieces* arena, const int64_t* item_idx_dev, int rows, int max_seq_len, int out_len,
                                        int n_sent, int n_span, const int32_t* special, const mdr_reader_train_batch* out, int device,
                                        void* stream) {
    using namespace mdr;
    const char* fn = "mdr_reader_train_compose";
    MDR_REQUIRE(rows >= 0 && out_len >= 1 && n_sent >= 0 && n_span >= 1, "%s: bad shape rows=%d out_len=%d n_sent=%d n_span=%d", fn, rows, out_len,
                n_sent, n_span);
    MDR_REQUIRE(arena && special && out, "%s: NULL pointer", fn);
    MDR_REQUIRE(arena->n_items >= 0 && arena->n_questions >= 0 && arena->n_passages >= 0 && arena->max_q_len >= 0,
                "%s: n_items=%lld n_questions=%lld n_passages=%lld max_q_len=%lld", fn, (long long)arena->n_items, (long long)arena->n_questions,
                (long long)arena->n_passages, (long long)arena->max_q_len);
    MDR_REQUIRE((long long)max_seq_len - (long long)arena->max_q_len >= 6, "%s: max_seq_len=%d leaves no room for yes no [SEP] after a question of %lld tokens",
                fn, max_seq_len, (long long)arena->max_q_len);
    if (rows == 0) return MDR_OK;
    MDR_REQUIRE(item_idx_dev, "%s: NULL item index", fn);
    MDR_REQUIRE(arena->n_items == 0 || (arena->q_offsets_dev && arena->p_offsets_dev && arena->p_sent_offsets_dev && arena->items_dev &&
                                        arena->sent_label_index_dev && arena->span_index_dev),
                "%s: NULL arena array", fn);
    MDR_REQUIRE(out->input_ids && out->attention_mask && out->token_type_ids && out->paragraph_mask && out->starts && out->ends && out->label &&
                    out->ans_covered && ((out->sent_offsets && out->sent_labels) || n_sent == 0),
                "%s: NULL output pointer", fn);
    DeviceGuard guard(device);
    if (!guard.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    mdr_reader_train_batch o = *out;
    if (n_sent == 0) o.sent_offsets = o.sent_labels = nullptr;
    ComposeSpecial sp{special[0], special[1], special[2], special[3], special[4]};
    hipLaunchKernelGGL(reader_train_compose_kernel, dim3(rows), dim3(kComposeThreads), 0, (hipStream_t)stream, *arena, (const long long*)item_idx_dev,
                       sp, max_seq_len, out_len, n_sent, n_span, o);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}
