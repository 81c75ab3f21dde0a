// csrc/mdr_mips.hip -- brute-force maximum-inner-product search for gfx950 (MI355X).
//
// Replaces faiss.IndexFlatIP.{add,search} as the reference's retrieval evaluation uses them (scripts/eval/eval_mhop_retrieval.py:121-122,155,179 there).
// See DESIGN.md §3-4 (layout, kernels) and NEGATIVE_RESULTS.md §3 (how they got there). This file holds the index handle and the C entry points; the
// kernels live in the section files included below, the host side of storage and search in mdr_mips_storage.inl and mdr_mips_search.inl.
//
// Storage (MDR_STORE_F32X2H). Every fp32 element x is kept as an fp16 pair
//     hi = fp16(x)            lo = fp16((x - hi) * 2^11)          x ~= hi + lo * 2^-11   (22-bit mantissa)
// = 4 bytes per element, the same HBM bytes as fp32, kept as TWO planes (all hi, all lo), each laid out
// in MFMA-operand order so that the HBM->LDS DMA and the LDS->register reads are perfectly linear:
//     plane -> row-block rb (16 rows) -> k-block kb (32 columns) -> 1 KiB fragment block
//     fragment block: lane l = (row & 15) + 16 * ((col & 31) >> 3) holds 8 consecutive columns (16 B)
// which is exactly the A/B operand layout of v_mfma_f32_16x16x32_f16.
//
// Search, k == 1, nq <= 128 per pass ("screen" kernel, the headline path): only the HI plane is
// streamed (2 bytes/element) and scored with ONE fp16 MFMA per k-block,  s_hi = qh.xh.  For every
// (q, x):  |q.x - qh.xh| <= B_q = 1.2e-3 * |q| * max_row|x|   (fp16 rounding of both operands, 2^-10,
// plus fp32 accumulation slack), so a row can only be the winner if  s_hi >= (largest s_hi seen) - 2 B_q.
// Those few rows (a handful per query: the running maxima and near-ties) are appended to a candidate
// list and re-scored exactly from both planes by mips_refine_kernel; if the list overflows (pathological
// all-ties corpora) a flag makes the exact 3-MFMA stream kernel below run instead. Results are identical
// to scoring every row exactly; HBM traffic is half the fp32 matrix.
//
// Search, nq <= 128 per pass ("stream" kernel): one 512-thread workgroup per CU, persistent over
// row-blocks. Wave w keeps the (hi, lo) fragments of queries 16w..16w+15 for ALL of K in registers
// (2 * NKB * 4 VGPRs), the corpus streams HBM -> LDS (global_load_lds, 3-deep ring of 1 row-block
// each) -> every wave's MFMA A operand. Three fp16 MFMAs per (row-block, k-block) give an
// fp32-accurate score:   q.x ~= qh.xh + (qh.xl + ql.xh) * 2^-11     (ql.xl ~ 2^-22 dropped)
// top-1 lives in two registers per lane; top-k (k <= 128) in per-wave candidate lists with a
// running threshold. The [nq, N] score matrix is never materialised.
#include <hip/hip_runtime.h>
#include <cstdlib>

#include <cfloat>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

#include "mdr_common.h"

namespace mdr {
namespace {

#include "mdr_mips_layout.inl"
#include "mdr_mips_exact.inl"
#include "mdr_mips_screen_fp16.inl"
#include "mdr_mips_generic.inl"
#ifndef MDR_MIPS_GEMMK
#define MDR_MIPS_GEMMK 0  // 1: measurement build that also holds the GEMM-structured beam > 1 main pass (mdr_mips_gemmk.inl; a measured negative of round 5)
#endif
#if MDR_MIPS_GEMMK
#include "mdr_mips_gemmk.inl"
#endif
#include "mdr_mips_screen_i8.inl"
#include "mdr_mips_merge.inl"

}  // namespace
}  // namespace mdr

// ---- host side ----
using namespace mdr;

struct mdr_index {
    int d = 0, nkb = 0, storage = 0, device = 0;
    int num_cus = 256;
    long long ntotal = 0;
    long long cap_rows = 0;  // multiple of 32 (one screen-kernel super-block)
    char* hi = nullptr;      // fragment-tiled planes, cap_rows * d * 2 bytes each
    char* lo = nullptr;
    char* i8 = nullptr;      // int8 screening plane (F32X2H storage, d = 768): cap_rows / 32 super-blocks of i8_sb_bytes(d / 64), see mips_screen8_kernel
    float* centre = nullptr; // [3 d] c | 1/w | w: centre and per-column scale of the int8 plane (col_sum_kernel), (0, 1, 1) until the first add() sets
                             // them, frozen afterwards; [3 d .. 5 d) scratch for the column sums
    bool centre_set = false;
    bool cb = false;         // the int8 tier scores the plane against q - lambda c (mdr_mips_screen_i8.inl "Query split"): decided with the centre (flags[11])
    bool terms_inf = false;  // a stored row's term b_r = c.(x_r - c) overflowed fp32 (flags[12], convert_to_i8_kernel): the query split stays off for good
    int xexp = 0;            // F32X2H: the planes hold x * 2^-xexp (see convert_to_frag_kernel); fitted to the data by add(), grown by a rescale
    bool xexp_set = false;
    int* flags = nullptr;    // device ints: [0] range error seen by add(), [1] same for queries (ignored), [2] max row |x|^2 (float bits),
                             // [8], [9], [10] int8 tier: max row scale, max s_r (L1(x8_r)/2 + d/4), max sum|c_i (x_i - c_i)| (float bits);
                             // [11] the centre is large against the rows' spread around it (centre_finish_kernel) -> cb;
                             // [12] a row's b_r or sum|c_i (x_i - c_i)| overflowed fp32 (convert_to_i8_kernel) -> terms_inf
    void* stage = nullptr;   // device staging for host-sourced add()
    size_t stage_bytes = 0;
    // pipelined host upload (upload_host_rows): two pinned staging buffers, a copy stream, "chunk copied" / "chunk converted" events per slot
    void* pin[2] = {nullptr, nullptr};
    size_t pin_bytes = 0;
    hipStream_t copy_st = nullptr;
    hipEvent_t ev_copy[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    int variant = 0;
    bool compact = false;    // MDR_STORE_F32X2H_COMPACT: no int8 screening plane
    const char* last_kernel = "none";
};

namespace {

#include "mdr_mips_storage.inl"
#include "mdr_mips_search.inl"

}  // namespace

extern "C" {

int mdr_index_create(int d, int storage, int device, mdr_index** out) {
    MDR_REQUIRE(out != nullptr, "out is NULL");
    MDR_REQUIRE(d > 0 && d % 32 == 0 && d <= 1024, "d=%d unsupported: must be a multiple of 32, <= 1024", d);
    MDR_REQUIRE(storage == MDR_STORE_F32X2H || storage == MDR_STORE_BF16 || storage == MDR_STORE_F32X2H_COMPACT, "unknown storage %d", storage);
    int ndev = 0;
    MDR_HIP_TRY(hipGetDeviceCount(&ndev));
    MDR_REQUIRE(device >= 0 && device < ndev, "device %d out of range (%d visible)", device, ndev);
    DeviceGuard g(device);
    if (!g.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    mdr_index* h = new (std::nothrow) mdr_index();
    MDR_REQUIRE(h != nullptr, "out of host memory");
    h->d = d;
    h->nkb = d / 32;
    h->storage = storage == MDR_STORE_F32X2H_COMPACT ? MDR_STORE_F32X2H : storage;
    h->compact = storage == MDR_STORE_F32X2H_COMPACT;
    h->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
    if (hipMalloc((void**)&h->flags, 256) != hipSuccess || hipMemset(h->flags, 0, 256) != hipSuccess) {
        delete h;
        return set_error(MDR_E_HIP, "hipMalloc(flags) failed");
    }
    *out = h;
    return MDR_OK;
}

int mdr_index_free(mdr_index* h) {
    if (!h) return MDR_OK;
    DeviceGuard g(h->device);
    if (h->hi) (void)hipFree(h->hi);
    if (h->lo) (void)hipFree(h->lo);
    if (h->i8) (void)hipFree(h->i8);
    if (h->centre) (void)hipFree(h->centre);
    if (h->flags) (void)hipFree(h->flags);
    if (h->stage) (void)hipFree(h->stage);
    for (int i = 0; i < 2; ++i) {
        if (h->pin[i]) (void)hipHostFree(h->pin[i]);
        if (h->ev_copy[i]) (void)hipEventDestroy(h->ev_copy[i]);
        if (h->ev_done[i]) (void)hipEventDestroy(h->ev_done[i]);
    }
    if (h->copy_st) (void)hipStreamDestroy(h->copy_st);
    delete h;
    return MDR_OK;
}

int mdr_index_reserve(mdr_index* h, int64_t n_rows) {
    MDR_REQUIRE(h != nullptr, "index handle is NULL");
    MDR_REQUIRE(n_rows >= 0 && n_rows < 0xFFFFFFE0ll, "n_rows out of range");
    DeviceGuard g(h->device);
    return grow(h, n_rows, nullptr);
}

int mdr_index_add(mdr_index* h, const void* rows, int64_t n, int src_dtype, int rows_on_device, void* stream) {
    MDR_REQUIRE(h != nullptr, "index handle is NULL");
    MDR_REQUIRE(n >= 0, "n < 0");
    MDR_REQUIRE(n == 0 || rows != nullptr, "rows is NULL");
    MDR_REQUIRE(src_dtype >= MDR_DT_F32 && src_dtype <= MDR_DT_F16, "unknown src_dtype %d", src_dtype);
    MDR_REQUIRE(h->ntotal + n < 0xFFFFFFE0ll, "index would exceed 2^32-32 rows per shard");
    if (n == 0) return MDR_OK;
    DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    int rc = grow(h, h->ntotal + n, st);
    if (rc) return rc;
    int before[16] = {0};  // [0..3] range / query / norm flags, [8..12] the int8 tier's row statistics, its query-split verdict and the row-term overflow: all restored when the rows are rejected
    const bool centre_was_set = h->centre_set;
    const int xexp_was = h->xexp;
    const bool xexp_was_set = h->xexp_set;
    MDR_HIP_TRY(hipMemcpyAsync(before, h->flags, sizeof(before), hipMemcpyDeviceToHost, st));
    MDR_HIP_TRY(hipStreamSynchronize(st));
    // ONE rollback for every failure from here on: a rejected add() -- in the first chunk or a later one, by the range check of
    // fit_exponent or by a conversion kernel's flag -- leaves the index exactly as it was: rows invisible (ntotal unchanged), norm / int8 statistics,
    // the int8 plane's centre and the exponent as before. (A rescale that an earlier chunk of the same call applied to the stored planes is exact
    // -- a power of two -- and stays; only the bookkeeping returns, so xexp is restored only when no rescale happened.)
    auto reject = [&](int code) {
        (void)hipMemcpyAsync(h->flags, before, sizeof(before), hipMemcpyHostToDevice, st);
        (void)hipStreamSynchronize(st);
        h->centre_set = centre_was_set;
        h->cb = before[11] != 0;
        h->terms_inf = before[12] != 0;
        if (!xexp_was_set) { h->xexp = xexp_was; h->xexp_set = false; }  // the exponent was fitted to rejected rows: forget it
        return code;
    };
    const size_t row_src = (size_t)h->d * elem_size(src_dtype);
    if (rows_on_device) {
        rc = add_any(h, rows, src_dtype, n, h->ntotal, st);
        if (rc) return reject(rc);
    } else {
        rc = upload_host_rows(h, (const char*)rows, n, src_dtype, row_src, st);
        if (rc) return reject(rc);
    }
    int after[16] = {0};
    MDR_HIP_TRY(hipMemcpyAsync(after, h->flags, sizeof(after), hipMemcpyDeviceToHost, st));
    MDR_HIP_TRY(hipStreamSynchronize(st));
    if (after[0]) return reject(set_error(MDR_E_RANGE, "add(): a value is non-finite; rows were not added"));
    h->cb = after[11] != 0;  // (written once, with the centre: centre_finish_kernel)
    h->terms_inf = after[12] != 0;
    h->ntotal += n;
    return MDR_OK;
}

int mdr_upload_host(void* dst_dev, const void* src_host, size_t bytes, int device, void* stream) {
    MDR_REQUIRE(bytes == 0 || (dst_dev && src_host), "NULL pointer");
    if (bytes == 0) return MDR_OK;
    DeviceGuard g(device);
    if (!g.ok) return set_error(MDR_E_HIP, "hipSetDevice(%d) failed", device);
    hipStream_t st = (hipStream_t)stream;
    const size_t chunk = 64ull << 20;
    if (bytes <= (4ull << 20)) {  // small: one plain copy
        MDR_HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, st));
        MDR_HIP_TRY(hipStreamSynchronize(st));
        return MDR_OK;
    }
    void* pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int rc = MDR_OK;
    auto fail = [&](const char* what) { rc = set_error(MDR_E_HIP, "%s failed in mdr_upload_host", what); };
    for (int i = 0; i < 2 && rc == MDR_OK; ++i) {
        if (hipHostMalloc(&pin[i], chunk, hipHostMallocDefault) != hipSuccess) fail("hipHostMalloc");
        else if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) fail("hipEventCreate");
    }
    const int nt = upload_threads();
    size_t off = 0;
    for (long long c = 0; rc == MDR_OK && off < bytes; ++c) {
        const int slot = (int)(c & 1);
        const size_t len = bytes - off < chunk ? bytes - off : chunk;
        if (c >= 2 && hipEventSynchronize(ev[slot]) != hipSuccess) { fail("hipEventSynchronize"); break; }  // the slot's previous copy has left the pinned buffer
        parallel_copy((char*)pin[slot], (const char*)src_host + off, len, nt);
        if (hipMemcpyAsync((char*)dst_dev + off, pin[slot], len, hipMemcpyHostToDevice, st) != hipSuccess) { fail("hipMemcpyAsync"); break; }
        if (hipEventRecord(ev[slot], st) != hipSuccess) { fail("hipEventRecord"); break; }
        off += len;
    }
    if (hipStreamSynchronize(st) != hipSuccess && rc == MDR_OK) fail("hipStreamSynchronize");
    for (int i = 0; i < 2; ++i) {
        if (ev[i]) (void)hipEventDestroy(ev[i]);
        if (pin[i]) (void)hipHostFree(pin[i]);
    }
    return rc;
}

int64_t mdr_index_ntotal(const mdr_index* h) { return h ? h->ntotal : 0; }
int mdr_index_dim(const mdr_index* h) { return h ? h->d : 0; }
int64_t mdr_index_stream_bytes(const mdr_index* h) { return h ? (int64_t)((h->ntotal + 15) / 16 * 16) * (int64_t)h->d * (is_bf16(h) ? 2 : 4) : 0; }

int mdr_index_set_variant(mdr_index* h, int variant) {
    MDR_REQUIRE(h != nullptr, "index handle is NULL");
    MDR_REQUIRE(variant >= 0 && variant <= (MDR_MIPS_GEMMK ? 5 : 4), "variant must be 0 (auto), 1 (generic), 2 (exact stream), 3 (screen + refine) or 4 (screen + refine "
                                                                      "without the int8 tier); 5 (GEMM-structured screen-k pass) exists in -DMDR_MIPS_GEMMK=1 builds only");
    h->variant = variant;
    return MDR_OK;
}

const char* mdr_index_last_kernel(const mdr_index* h) { return h ? h->last_kernel : "none"; }

int mdr_index_queries_per_pass(const mdr_index* h, int nq, int k) {
    if (!h || k < 1 || k > kKMax || nq < 1) return 0;
    const int path = make_plan(h, nq, k).path;
    if (path == PATH_GENERIC) return kGenericQ;
    return path == PATH_SCREEN && wide_pass(nq) ? kWideQ : kStreamQ;
}

size_t mdr_index_search_workspace_bytes(const mdr_index* h, int nq, int k) {
    if (!h || nq < 0 || k < 1 || k > kKMax) return 0;
    return make_plan(h, nq, k).total;
}

int mdr_index_search(mdr_index* h, const float* q_dev, int nq, int k, float* D_dev, int64_t* I_dev, int64_t id_offset, void* workspace_dev,
                     size_t workspace_bytes, void* stream) {
    MDR_REQUIRE(h != nullptr, "index handle is NULL");
    MDR_REQUIRE(nq >= 0, "nq < 0");
    MDR_REQUIRE(k >= 1 && k <= kKMax, "k=%d out of range [1, %d]", k, kKMax);
    if (nq == 0) return MDR_OK;
    MDR_REQUIRE(q_dev && D_dev && I_dev, "NULL query/result pointer");
    if (h->variant == PATH_STREAM && !stream_kernel_supports(h, k))
        return set_error(MDR_E_INVALID, "stream kernel forced but unsupported for d=%d k=%d storage=%d (needs F32X2H, d=768, k<=128)", h->d, k, h->storage);
    if (h->variant == PATH_SCREEN && !screen_kernel_supports(h, k))
        return set_error(MDR_E_INVALID, "screen kernel forced but unsupported for d=%d k=%d (needs d=768, k<=256)", h->d, k);
    DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    long long* I_ll = (long long*)I_dev;
    if (h->ntotal == 0) {
        long long n = (long long)nq * k;
        hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, D_dev, I_ll, n);
        MDR_HIP_TRY(hipGetLastError());
        h->last_kernel = "fill_empty_kernel";
        return MDR_OK;
    }
    const SearchPlan p = make_plan(h, nq, k);
    if (!workspace_dev || workspace_bytes < p.total)
        return set_error(MDR_E_WORKSPACE, "workspace too small: need %zu bytes, got %zu", p.total, workspace_bytes);
    char* ws = (char*)(((uintptr_t)workspace_dev + 255) & ~(uintptr_t)255);
    h->last_kernel = search_kernel_name(h, p, nq, k);
    if (p.path == PATH_GENERIC) return run_generic(h, p, ws, q_dev, nq, k, D_dev, I_ll, id_offset, nullptr, st);
    int rc = prep_queries(h, p, ws, q_dev, nq, k, st);
    if (rc) return rc;
    const bool bf = is_bf16(h), wide = wide_pass(nq), screen = p.path == PATH_SCREEN;
    // the exact pass behind a screen runs only if one of its candidate lists (k > 1: or the band) overflowed; on the stream path it is the search
    const int* run_if = screen ? (const int*)(ws + p.off_sctl) : nullptr;

    if (k == 1) {
        u64* best = (u64*)(ws + p.off_best);
        if (screen) MDR_HIP_TRY(hipMemsetAsync(ws + p.off_zero, 0, p.zero_bytes, st));  // best + every tier's control words, one node
        else MDR_HIP_TRY(hipMemsetAsync(best, 0, (size_t)nq * 8, st));
        if (screen) {  // the int8 tier first where the plan has it; behind it the fp16 screen only if one of ITS lists overflowed (ctl8[0])
            if (p.i8) rc = dispatch(wide, use_cb(h), [&](auto w, auto cb) { return run_screen8(w, cb, h, p, ws, q_dev, nq, st); });
            if (!rc) rc = dispatch(wide, bf, [&](auto w, auto b) { return run_screen(w, b, h, p, ws, q_dev, nq, st, p.i8 ? (const int*)(ws + p.off_ctl8) : nullptr); });
            if (rc) return rc;
        }
        if (!bf) rc = run_stream_top1(h, p, ws, nq, run_if, st);
        if (rc) return rc;
        hipLaunchKernelGGL(finalize_top1_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, (const u64*)best, nq, D_dev, I_ll, (long long)id_offset);
        MDR_HIP_TRY(hipGetLastError());
        // bf16 storage has no exact MFMA pass: the overflow fallback is the generic kernel, overwriting D/I
        return bf ? run_generic(h, p, ws, q_dev, nq, 1, D_dev, I_ll, id_offset, run_if, st) : MDR_OK;
    }

    // 2 <= k <= 256 (screen path; the exact stream kernel behind / instead of it serves F32X2H rows up to k = 128, the generic kernel the rest)
    if (screen) {
        rc = dispatch(wide, bf, [&](auto w, auto b) { return run_screenk(w, b, h, p, ws, q_dev, nq, k, D_dev, I_ll, id_offset, st); });
        if (rc) return rc;
        if (!stream_kernel_supports(h, k)) return run_generic(h, p, ws, q_dev, nq, k, D_dev, I_ll, id_offset, run_if, st);
    }
    return run_stream_topk(h, p, ws, nq, k, D_dev, I_ll, id_offset, run_if, st);
}

#if MDR_I8_ABL == 9  // measurement builds only (include/mdr_hip_measure.h)
int mdr_test_i8_stamps(unsigned long long* out8_host, int reset) {
    MDR_REQUIRE(out8_host, "NULL pointer");
    MDR_HIP_TRY(hipDeviceSynchronize());
    MDR_HIP_TRY(hipMemcpyFromSymbol(out8_host, HIP_SYMBOL(g_i8_stamp), 8 * sizeof(unsigned long long)));
    if (reset) {
        const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        MDR_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_i8_stamp), z, sizeof(z)));
    }
    return MDR_OK;
}
#endif

int mdr_index_search_telemetry(const mdr_index* h, int nq, int k, const void* workspace_dev, int64_t* out4_host, void* stream) {
    MDR_REQUIRE(h && workspace_dev && out4_host, "NULL argument");
    MDR_REQUIRE(nq >= 1 && k >= 1 && k <= kKMax, "bad shape");
    DeviceGuard g(h->device);
    hipStream_t st = (hipStream_t)stream;
    const SearchPlan p = make_plan(h, nq, k);
    const char* ws = (const char*)(((uintptr_t)workspace_dev + 255) & ~(uintptr_t)255);
    out4_host[0] = out4_host[1] = out4_host[2] = 0;
    out4_host[3] = p.path;
    // every word of the report is copied first, then ONE sync
    int flags[4] = {0, 0, 0, 0}, sctl[2] = {0, 0}, ctl8[2] = {0, 0};  // sctl: [0] overflow, [1] k > 1: merge_screenk_kernel adds every query's union size; ctl8: [0] overflow, [1] re-scored
    const size_t n_cnt = p.path == PATH_SCREEN && k == 1 ? (size_t)(p.i8 ? (wide_pass(nq) ? p.G8w : p.G8) : p.G) * 8 : 0;  // k == 1: per-wave list lengths of the last query group
    std::unique_ptr<int[]> cnt(new (std::nothrow) int[n_cnt]);
    MDR_REQUIRE(cnt != nullptr, "out of host memory");
    MDR_HIP_TRY(hipMemcpyAsync(flags, h->flags, sizeof(flags), hipMemcpyDeviceToHost, st));
    if (p.path == PATH_SCREEN) MDR_HIP_TRY(hipMemcpyAsync(sctl, ws + p.off_sctl, sizeof(sctl), hipMemcpyDeviceToHost, st));
    if (n_cnt) MDR_HIP_TRY(hipMemcpyAsync(cnt.get(), ws + p.off_sctl + 256, n_cnt * sizeof(int), hipMemcpyDeviceToHost, st));
    if (p.i8) MDR_HIP_TRY(hipMemcpyAsync(ctl8, ws + p.off_ctl8, sizeof(ctl8), hipMemcpyDeviceToHost, st));
    MDR_HIP_TRY(hipStreamSynchronize(st));
    out4_host[2] = flags[1];
    if (p.path != PATH_SCREEN) return MDR_OK;
    long long total = sctl[1];
    if (k == 1) {
        total = 0;
        for (size_t i = 0; i < n_cnt; ++i) total += cnt[i];
    }
    out4_host[0] = sctl[0];
    out4_host[1] = total;
    // bit 9: the int8 tier ran in front; bit 8: one of its lists overflowed (the fp16 screen ran behind it); bit 10: the query split is on;
    // bits 16..: candidates of the int8 tier that were really re-scored
    if (p.i8) out4_host[3] |= 512 | (ctl8[0] ? 256 : 0) | (use_cb(h) ? 1024 : 0) | ((int64_t)ctl8[1] << 16);
    return MDR_OK;
}

int mdr_topk_merge(const float* D_parts_dev, const int64_t* I_parts_dev, int nparts, int nq, int k, float* D_dev, int64_t* I_dev, void* stream) {
    MDR_REQUIRE(nparts >= 1 && nq >= 0 && k >= 1 && k <= kKMax, "bad merge shape nparts=%d nq=%d k=%d", nparts, nq, k);
    if (nq == 0) return MDR_OK;
    MDR_REQUIRE(D_parts_dev && I_parts_dev && D_dev && I_dev, "NULL pointer");
    hipLaunchKernelGGL(merge_parts_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, D_parts_dev, (const long long*)I_parts_dev, nparts, nq, k, D_dev,
                       (long long*)I_dev);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

size_t mdr_topk_packed_ids_offset(int nq, int k) {
    if (nq < 0 || k < 1) return 0;
    return align_up((size_t)nq * (size_t)k * 4, 8);
}

size_t mdr_topk_packed_bytes(int nq, int k) {
    if (nq < 0 || k < 1) return 0;
    return align_up(mdr_topk_packed_ids_offset(nq, k) + (size_t)nq * (size_t)k * 8, 256);
}

int mdr_topk_merge_packed(const void* packed_parts_dev, int nparts, int nq, int k, float* D_dev, int64_t* I_dev, void* stream) {
    MDR_REQUIRE(nparts >= 1 && nq >= 0 && k >= 1 && k <= kKMax, "bad merge shape nparts=%d nq=%d k=%d", nparts, nq, k);
    if (nq == 0) return MDR_OK;
    MDR_REQUIRE(packed_parts_dev && D_dev && I_dev, "NULL pointer");
    MDR_REQUIRE(((uintptr_t)packed_parts_dev & 7) == 0, "packed blocks must be 8-byte aligned");
    hipLaunchKernelGGL(merge_packed_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, (const char*)packed_parts_dev, (long long)mdr_topk_packed_bytes(nq, k),
                       (long long)mdr_topk_packed_ids_offset(nq, k), nparts, nq, k, D_dev, (long long*)I_dev);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

}  // extern "C"
