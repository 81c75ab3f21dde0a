// csrc/mdr_mips_search.inl -- host side of a search call: the schedule knobs, the plan (path, grids, workspace layout) and one driver per
// path that launches its kernels. Included by mdr_mips.hip inside its unnamed namespace, after mdr_mips_storage.inl.

// MDR_MIPS_WIDE=0 keeps every call on the 128-queries-per-pass kernels (measurement knob)
bool wide_pass(int nq) {
    static const bool off = getenv("MDR_MIPS_WIDE") && atoi(getenv("MDR_MIPS_WIDE")) == 0;
    return !off && nq > kStreamQ;
}
// The GEMM-structured main pass of the beam > 1 search (mdr_mips_gemmk.inl) is a MEASURED NEGATIVE of round 5 (four versions, 2.7-2.9 ms per 256-query pass at
// 5 M rows where mips_screenk32_kernel takes 2.3-2.4; NEGATIVE_RESULTS round 5). The product library does not contain it (round 6); a -DMDR_MIPS_GEMMK=1 build does
// and runs it for test-hook variant 5 (tests/test_mips_gpu.py keeps it honest there: same lists, same bits) or with MDR_MIPS_GEMMK=1 in the environment (A/B runs).
bool gemmk_on(const mdr_index* h) {
#if MDR_MIPS_GEMMK
    static const bool env_on = getenv("MDR_MIPS_GEMMK") && atoi(getenv("MDR_MIPS_GEMMK")) == 1;
    return env_on || h->variant == 5;
#else
    (void)h;
    return false;
#endif
}
// Query groups of a call with more than kWideQ queries on the 32-queries-per-wave kernels (round 6). VERDICT r5 item 4 asked for the ceil(nq / 256) passes to share the
// ceil(nq / 32) waves EVENLY instead of 256 + 256 + ... + rest (nq 300 = 160 + 140 instead of 256 + 44, nq 800 = 224 + 3 x 192 instead of 3 x 256 + 32), on the model that a pass
// costs its active waves down to the HBM floor. Measured (profiles/r06_query_groups_ab.txt, r06_query_groups_k_sweep.txt): results bit-identical, time within +-4 % -- a pass costs
// its HBM time PLUS a per-wave term that is the clock falling under matrix-pipe load (profiles/r06_screenk32_overlap_ablation_and_clock.txt), so moving waves between passes moves
// little. What is left is a k-dependence: nq 800 at 6.25 M bf16 rows, even vs old cut: k 8 / 16: -2 %, k 32: equal, k 64: +2 %, k 100: +4 %; 5 M fp32-accurate rows: k 8 -2.5 %,
// k 100 +2.5 %, k 1 +1 % (with long lists the 32-query remainder is cheapest on the 16-queries-per-wave kernels). Rule: the even cut for 2 <= k <= 32, the old cut otherwise.
// Every buffer the groups index (query fragments in 16-query blocks, bounds, thresholds, best, outputs) is linear in the query number, so a group is just (first query, count)
// with the first a multiple of 32. MDR_MIPS_EVEN_GROUPS: 0 = the old cut always, 1 (default) = the rule, 2 = even + groups of <= 128 queries on the 16-queries-per-wave
// kernels, 3 = the even cut always (A/B runs and tests; same results in every mode).
int even_groups_mode() {
    static const int m = getenv("MDR_MIPS_EVEN_GROUPS") ? atoi(getenv("MDR_MIPS_EVEN_GROUPS")) : 1;
    return m;
}
bool even_cut(int k) {
    const int m = even_groups_mode();
    return m >= 2 || (m == 1 && k >= 2 && k <= 32);
}
struct QGroup { int q0, n; };
int group_count(int per_pass, int nq) { return (nq + per_pass - 1) / per_pass; }
// group gi of a call of nq queries on kernels that serve `per_pass` queries per corpus pass: the even cut is a matter of the 32-queries-per-wave kernels
QGroup query_group(int per_pass, int nq, int gi, int k) {
    if (per_pass == kStreamQ || !even_cut(k)) return {gi * per_pass, nq - gi * per_pass < per_pass ? nq - gi * per_pass : per_pass};
    const int ng = group_count(kWideQ, nq), waves = (nq + 31) / 32;
    const int base = waves / ng, extra = waves % ng;
    const int w0 = gi * base + (gi < extra ? gi : extra), w1 = w0 + base + (gi < extra ? 1 : 0);
    const int end = w1 * 32 < nq ? w1 * 32 : nq;
    return {w0 * 32, end - w0 * 32};
}
bool stream_kernel_supports(const mdr_index* h, int k) { return !is_bf16(h) && h->d == 768 && k <= 128; }
bool screen_kernel_supports(const mdr_index* h, int k) { return h->d == 768 && k <= 256; }
// sample stages per workgroup of the k > 1 screen (mips_screen_kernel MODE 2): one published maximum per stage
int sample_stages_for(int k) { return k > 128 ? 2 * kSampleStagesK : kSampleStagesK; }

enum Path { PATH_GENERIC = 1, PATH_STREAM = 2, PATH_SCREEN = 3 };

struct SearchPlan {
    int path;
    int G;    // workgroups of the stream / screen kernels
    int Gx;   // workgroups of the exact stream kernel (== G on the stream path; the fallback behind the screen kernels)
    int Gg;   // workgroups of the generic kernel (when its lists are needed)
    bool lists_stream, lists_generic;
    size_t off_qhi, off_qlo, off_bound, off_qscale, off_best, off_gmax, off_scand, off_sctl, off_cand, off_cnt, off_kth, total;
    bool i8;  // the int8 screening tier runs in front of the fp16 screen (k == 1)
    int G8w;  // workgroups of its 32-queries-per-wave kernel
    int G8;   // its workgroups: TWO per CU (24.25 KiB super-blocks: three slots are 73 KiB), one's barrier and epilogue under the other's MFMAs.
              // Measured at 5 M rows, planted queries, whole call: 1 per CU 1.013 ms, 1 per CU with 64-row stages 0.995 ms, 2 per CU 0.907 ms.
    size_t off_q8, off_qab, off_qlam, off_ctl8, off_gstar;
    size_t off_zero, zero_bytes, off_gmax_b;  // the k = 1 screen path's zero block (make_plan)
};

#ifndef MDR_I8W_SLOTS
#define MDR_I8W_SLOTS 3  // the 32-queries-per-wave int8 kernel needs > 128 VGPRs: ONE workgroup per CU; its stages are 64 rows (48.5 KiB), two in flight
#endif
#ifndef MDR_I8_SLOTS
#define MDR_I8_SLOTS 3  // variant-build knob: LDS ring depth of the int8 screen kernels (3: two workgroups per CU, 4-6: one)
#endif
// variant 4 = the screen path WITHOUT the int8 tier (tests and A/B runs)
// (the tier's 16-queries-per-wave kernels serve ONE group of at most kStreamQ queries; more than that goes to the 32-queries-per-wave kernels
// in groups of 256 -- or, with MDR_MIPS_WIDE=0, stays on the fp16 screen in groups of 128: i8_tier)
// MDR_MIPS_I8_CB = 0 / 1 forces the query split of the int8 tier off / on (A/B runs; results are the same either way: any lambda is correct)
// -- except on an index with a row whose term b_r overflowed fp32 (terms_inf: finite rows with |x| |c| beyond 3.4e38, added after the rows that set
// the centre c): that row's split bound is NaN and would never make it a candidate, so the split is off there whatever the index or the variable says.
// The non-split kernels never read b_r.
bool use_cb(const mdr_index* h) {
    static const int force = getenv("MDR_MIPS_I8_CB") ? atoi(getenv("MDR_MIPS_I8_CB")) : -1;
    if (h->terms_inf) return false;
    return force < 0 ? h->cb : force != 0;
}
bool i8_tier(const mdr_index* h, int path, int nq, int k) {
    return h->i8 != nullptr && h->variant != 4 && path == PATH_SCREEN && k == 1 && nq < 65536 && (nq <= kStreamQ || wide_pass(nq));
}

// workgroups for `units` units of work on a device that runs `cap` of them at once: never an empty grid
int clamp_grid(long long units, long long cap) { return (int)(units < cap ? (units > 0 ? units : 1) : cap); }

SearchPlan make_plan(const mdr_index* h, int nq, int k) {
    SearchPlan p{};
    const int v = h->variant;
    if (v == PATH_GENERIC) p.path = PATH_GENERIC;
    else if (v == PATH_STREAM) p.path = stream_kernel_supports(h, k) ? PATH_STREAM : PATH_GENERIC;
    else if (screen_kernel_supports(h, k)) p.path = PATH_SCREEN;  // auto or forced screen
    else if (stream_kernel_supports(h, k)) p.path = PATH_STREAM;
    else p.path = PATH_GENERIC;
    const long long n_rb = (h->ntotal + 15) / 16;
    const long long units = p.path == PATH_SCREEN ? (h->ntotal + 31) / 32 : n_rb;
    p.G = clamp_grid(units, h->num_cus);
    if (p.G > 1024) p.G = 1024;
    p.Gx = clamp_grid(n_rb, h->num_cus);
    p.Gg = clamp_grid(n_rb, (long long)h->num_cus * 2);
    // which candidate-list workspaces this call can touch (incl. the conditional exact pass behind the screen kernel)
    // (the exact pass behind the screen-k kernels: the MFMA stream kernel up to its k = 128, the generic kernel for bf16 rows and for 128 < k <= 256)
    p.lists_stream = (p.path == PATH_STREAM || (p.path == PATH_SCREEN && !is_bf16(h) && stream_kernel_supports(h, k))) && k > 1;
    p.lists_generic = p.path == PATH_GENERIC || (p.path == PATH_SCREEN && (is_bf16(h) || !stream_kernel_supports(h, k)));
    const bool screenk = p.path == PATH_SCREEN && k > 1;
    const bool frag = p.path != PATH_GENERIC;
    const size_t nq_pad = (size_t)((nq + kWideQ - 1) / kWideQ) * kWideQ;  // covers both group sizes (128 and 256 queries per pass)
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += align_up(bytes, 256); return at; };
    p.off_qhi = take(frag ? nq_pad * h->d * 2 : 0);
    p.off_qlo = take(frag && !is_bf16(h) ? nq_pad * h->d * 2 : 0);
    p.off_bound = take(frag ? nq_pad * 4 : 0);
    p.off_qscale = take(frag ? nq_pad * 4 : 0);
    // ---- the k = 1 screen path's zero block: everything its tiers expect cleared, contiguous, ONE memset per search call (round 5: seven memset nodes
    // between the kernels of a 0.9 ms call were seven ~1.5 us boundaries): best | gmax | gmax_b | gstar | ctl8 | sctl ----
    p.i8 = i8_tier(h, p.path, nq, k);
    p.off_best = take((size_t)(nq > 0 ? nq : 1) * 8);
    p.off_zero = p.off_best;
    p.off_gmax = take(p.path == PATH_SCREEN ? nq_pad * 4 : 0);
    p.off_gmax_b = take(p.path == PATH_SCREEN && p.i8 ? nq_pad * 4 : 0);  // the fp16 tier's sample maxima when it runs BEHIND the int8 tier (which owns gmax)
    p.off_gstar = take(p.i8 ? nq_pad * 8 : 0);
    p.off_ctl8 = take(p.i8 ? 256 : 0);  // [0] a candidate list of the int8 tier overflowed -> the fp16 screen runs
    // k == 1: one private list per wave; k > 1: the [G][kStreamQ] sample maxima
    p.G8 = clamp_grid(units, (MDR_I8_SLOTS <= 3 ? 2ll : 1ll) * h->num_cus);  // workgroups of the int8 kernels per CU: two with 3 LDS slots (73 KiB), one with 4-6 (146 KiB)
    p.G8w = clamp_grid((units + 1) / 2, h->num_cus);                         // the 32-queries-per-wave kernel: one per CU, stages of two super-blocks
    const size_t gl = p.i8 && p.G8 > p.G ? (size_t)p.G8 : (size_t)p.G;  // workgroups that own candidate lists
    p.off_sctl = take(p.path == PATH_SCREEN ? 256 + gl * 8 * 4 : 0);            // [0] overflow flag, [64..] per-wave counts
    p.zero_bytes = p.off_sctl + (p.path == PATH_SCREEN ? 256 : 0) - p.off_zero;  // (the per-wave counts behind the head are written before they are read)
    p.off_scand = take(p.path != PATH_SCREEN ? 0 : (k == 1 ? gl * 8 * kWaveCandCap * 8 : (size_t)p.G * sample_stages_for(k) * kWideQ * 4));
    // the screen-k lists and the lists of its conditional exact pass (which runs after them in stream order) share one region
    size_t lists = p.lists_stream ? (size_t)p.Gx * kStreamQ * kStreamCap : (p.lists_generic ? (size_t)p.Gg * kGenericQ * kGenericCap : 0);
    size_t slots = p.lists_stream ? (size_t)p.Gx * kStreamQ : (p.lists_generic ? (size_t)p.Gg * kGenericQ : 0);
    if (screenk) {
        const size_t qc = wide_pass(nq) ? kWideQ : kStreamQ;
        const size_t l2 = (size_t)p.G * qc * kScreenKCap, s2 = (size_t)p.G * qc;
        lists = lists > l2 ? lists : l2;
        slots = slots > s2 ? slots : s2;
    }
    p.off_cand = take(lists * 8);
    p.off_cnt = take(slots * 4);
    p.off_kth = take(slots * 8);
    p.off_q8 = take(p.i8 ? nq_pad * h->d : 0);
    p.off_qab = take(p.i8 ? nq_pad * 16 : 0);
    p.off_qlam = take(p.i8 ? nq_pad * 4 : 0);  // lambda_q of the query split
    p.total = o + 256;
    return p;
}

// ---- width descriptors: the screened paths exist in two widths whose kernels take the same parameter lists ----
constexpr int kNkb = 24, kNkb8 = 12;                             // d = 768 in k-blocks of 32 fp16 / 64 int8 columns
constexpr size_t kStageBytes = (size_t)kNkb * 2 * kFragBytes;    // one LDS stage of the exact and the fp16 screen kernels: 48 KiB
constexpr size_t kScreenLds = 3 * kStageBytes;
constexpr size_t kMergeKLdsBytes = (size_t)kMergeKLds * 8;
constexpr size_t kI8SbLds = 2 * kNkb8 * kFragBytes + kI8Tail;    // one super-block of the int8 plane in LDS
#if MDR_MIPS_GEMMK
constexpr size_t kGemmkLds = (4 + 4) * 16 * kFragBytes + kWideQ * 8;  // four row-fragment + four query-fragment slots of 16 KiB, list counters, thresholds
#endif

struct Narrow {  // 16 queries per wave
    static constexpr int kQ = kStreamQ;                               // queries per corpus pass = stride of the per-query lists
    static constexpr int kI8Slots = MDR_I8_SLOTS, kI8SbPerSlot = 1;   // LDS ring of the int8 kernel
    static int i8_grid(const SearchPlan& p) { return p.G8; }
    template <int MODE, bool BF> static constexpr auto screen() { return &mips_screen_kernel<kNkb, MODE, BF>; }
    template <bool BF> static constexpr auto screenk() { return &mips_screenk_kernel<kNkb, BF>; }
    template <int MODE, bool CB> static constexpr auto screen8() { return &mips_screen8_kernel<kNkb8, MODE, kI8Slots, CB>; }
};
struct Wide {  // 32 queries per wave
    static constexpr int kQ = kWideQ;
    static constexpr int kI8Slots = MDR_I8W_SLOTS, kI8SbPerSlot = 2;  // a stage of this kernel = two super-blocks
    static int i8_grid(const SearchPlan& p) { return p.G8w; }
    template <int MODE, bool BF> static constexpr auto screen() { return &mips_screen32_kernel<kNkb, MODE, BF>; }
    template <bool BF> static constexpr auto screenk() { return &mips_screenk32_kernel<kNkb, BF>; }
    template <int MODE, bool CB> static constexpr auto screen8() { return &mips_screen8w_kernel<kNkb8, MODE, kI8Slots, CB>; }
};
template <bool B> using Flag = std::integral_constant<bool, B>;
// runtime (wide, flag) -> the width descriptor and the BF / CB template argument of a driver: f(Narrow or Wide, Flag<false> or Flag<true>)
template <class F>
int dispatch(bool wide, bool flag, F f) {
    if (wide) return flag ? f(Wide{}, Flag<true>{}) : f(Wide{}, Flag<false>{});
    return flag ? f(Narrow{}, Flag<true>{}) : f(Narrow{}, Flag<false>{});
}

// the GEMM-structured main pass takes a wide screen-k group's place (measurement builds only; it reads whole 256-row tiles per workgroup)
bool gemmk_runs(const mdr_index* h, const SearchPlan& p) { return gemmk_on(h) && h->ntotal >= 256ll * p.G; }

// what mdr_index_last_kernel() reports for a call with this plan: the kernel that decides it when no list overflows
const char* search_kernel_name(const mdr_index* h, const SearchPlan& p, int nq, int k) {
    const bool bf = is_bf16(h), wide = wide_pass(nq);
    if (p.path == PATH_GENERIC) return "mips_generic_kernel";
    if (p.path == PATH_STREAM) return k == 1 ? "mips_stream_kernel<24,0>" : "mips_stream_kernel<24,1>";
    if (k == 1 && p.i8) return wide ? "mips_screen8w_kernel<12,1>" : "mips_screen8_kernel<12,1>";
    if (k == 1 && wide) return bf ? "mips_screen32_kernel<24,1,bf16>" : "mips_screen32_kernel<24,1>";
    if (k == 1) return bf ? "mips_screen_kernel<24,1,bf16>" : "mips_screen_kernel<24,1>";
    if (wide && gemmk_runs(h, p)) return bf ? "mips_gemmk_kernel<bf16>" : "mips_gemmk_kernel";
    if (wide) return bf ? "mips_screenk32_kernel<24,bf16>" : "mips_screenk32_kernel<24>";
    return bf ? "mips_screenk_kernel<24,bf16>" : "mips_screenk_kernel<24>";
}

// query fragments (fp16 hi / lo, for the int8 tier also the int8 queries and their constants), screen bounds and scales of every query of the call
int prep_queries(mdr_index* h, const SearchPlan& p, char* ws, const float* q_dev, int nq, int k, hipStream_t st) {
    // |q.x - qh.xh| <= c |q| max|x|: fp16 rounding of both operands (2^-10) or bf16 rounding of q only (2^-9; the
    // stored rows ARE the bf16 values), plus fp32 accumulation slack
    const bool bf = is_bf16(h);
    const float c = bf ? 2.2e-3f : 1.2e-3f;
    const int nq_pad = group_count(kWideQ, nq) * kWideQ;
    char *qhi = ws + p.off_qhi, *qlo = ws + p.off_qlo;
    float *bound = (float*)(ws + p.off_bound), *qscale = (float*)(ws + p.off_qscale);
    MDR_HIP_TRY(hipMemsetAsync(h->flags + 1, 0, sizeof(int), st));  // "a query of THIS call was non-finite" (telemetry)
    if (bf)
        hipLaunchKernelGGL((prep_queries_kernel<true>), dim3((nq_pad + 3) / 4), dim3(256), 0, st, q_dev, nq, nq_pad, h->d, h->flags, c, qhi, qlo, bound, qscale, 1.0f);
    else if (p.i8 && k == 1) {
        const int nq_pad8 = wide_pass(nq) ? nq_pad : kStreamQ;  // what run_screen8 reads: whole groups of 256 / one group of 128 queries
        const int nb16 = (nq_pad + 3) / 4, nb8 = (nq_pad8 + 3) / 4;
        hipLaunchKernelGGL(prep_queries_both_kernel, dim3(nb16 + nb8), dim3(256), 0, st, nb16, q_dev, nq, nq_pad, nq_pad8, h->d, h->flags, c, qhi, qlo, bound, qscale,
                           row_unscale(h), ws + p.off_q8, (f32x4*)(ws + p.off_qab), (const float*)h->centre, (int)use_cb(h), (float*)(ws + p.off_qlam));
    } else
        hipLaunchKernelGGL((prep_queries_kernel<false>), dim3((nq_pad + 3) / 4), dim3(256), 0, st, q_dev, nq, nq_pad, h->d, h->flags, c, qhi, qlo, bound, qscale,
                           row_unscale(h));
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

// generic kernel + merge over all queries in groups of kGenericQ; every launch is skipped on the device when *run_if == 0
int run_generic(mdr_index* h, const SearchPlan& p, char* ws, const float* q_dev, int nq, int k, float* D_dev, long long* I_dev, long long id_offset,
                const int* run_if, hipStream_t st) {
    const auto kern = is_bf16(h) ? &mips_generic_kernel<true> : &mips_generic_kernel<false>;
    u64* cand = (u64*)(ws + p.off_cand);
    int* cnt = (int*)(ws + p.off_cnt);
    u64* kth = (u64*)(ws + p.off_kth);
    const int n_rb = (int)((h->ntotal + 15) / 16);
    for (int q0 = 0; q0 < nq; q0 += kGenericQ) {
        const int nqg = nq - q0 < kGenericQ ? nq - q0 : kGenericQ;
        MDR_HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)p.Gg * kGenericQ * 4, st));
        MDR_HIP_TRY(hipMemsetAsync(kth, 0, (size_t)p.Gg * kGenericQ * 8, st));
        hipLaunchKernelGGL(kern, dim3(p.Gg), dim3(256), 0, st, (const char*)h->hi, (const char*)h->lo, (long long)h->ntotal, n_rb, h->nkb,
                           q_dev + (size_t)q0 * h->d, nqg, cand, cnt, kth, k, run_if, row_unscale(h));
        hipLaunchKernelGGL(merge_lists_kernel, dim3(nqg), dim3(256), 0, st, (const u64*)cand, (const int*)cnt, (const u64*)kth, p.Gg, kGenericQ, kGenericCap,
                           k, D_dev + (size_t)q0 * k, I_dev + (size_t)q0 * k, id_offset, run_if, (const float*)nullptr);
        MDR_HIP_TRY(hipGetLastError());
    }
    return MDR_OK;
}

// k == 1, the fp16 tier: sample pass, main pass, exact re-scoring of the candidates, per query group. run_if: behind the int8 tier, whose
// overflow word lets it run (it then keeps its own sample maxima; both sets are part of the call's zero block, as is sctl[0..63])
template <class W, bool BF>
int run_screen(W, Flag<BF>, mdr_index* h, const SearchPlan& p, char* ws, const float* q_dev, int nq, hipStream_t st, const int* run_if) {
    const auto passes = {W::template screen<0, BF>(), W::template screen<1, BF>()};
    for (auto pass : passes)
        if (int rc = ensure_dynamic_lds((const void*)pass, (int)kScreenLds)) return rc;
    const char* qhi = ws + p.off_qhi;
    const float* bound = (const float*)(ws + p.off_bound);
    unsigned* gmax = (unsigned*)(ws + (run_if && p.i8 ? p.off_gmax_b : p.off_gmax));
    u64 *scand = (u64*)(ws + p.off_scand), *best = (u64*)(ws + p.off_best);
    int* sctl = (int*)(ws + p.off_sctl);
    int* wave_cnt = sctl + 64;
    const int n_sb = (int)((h->ntotal + 31) / 32);
    for (int gi = 0; gi < group_count(W::kQ, nq); ++gi) {
        const QGroup g = query_group(W::kQ, nq, gi, 1);
        for (auto pass : passes)
            hipLaunchKernelGGL(pass, dim3(p.G), dim3(512), kScreenLds, st, (const char*)h->hi, (long long)h->ntotal, n_sb, qhi + (size_t)g.q0 * h->d * 2,
                               bound + g.q0, g.n, g.q0, gmax + g.q0, scand, wave_cnt, sctl, run_if, kSampleStagesK);
        hipLaunchKernelGGL((mips_refine_kernel<BF>), dim3(p.G * 8), dim3(256), 0, st, (const char*)h->hi, (const char*)h->lo, h->nkb, q_dev,
                           (const u64*)scand, (const int*)wave_cnt, best, row_unscale(h), run_if);
        MDR_HIP_TRY(hipGetLastError());
    }
    return MDR_OK;
}

// k == 1, int8 plane present: the int8 tier per query group -- sample pass and main pass, each followed by the exact re-scoring of its
// best-lower-bound rows (a first `known` that is up to 2 B tighter than their lower bounds), then the exact re-scoring of the candidates.
// (gmax, gstar and ctl8 are part of the call's zero block; q8 / qab / qlam were written by prep_queries)
template <class W, bool CB>
int run_screen8(W, Flag<CB>, mdr_index* h, const SearchPlan& p, char* ws, const float* q_dev, int nq, hipStream_t st) {
    const auto passes = {W::template screen8<0, CB>(), W::template screen8<1, CB>()};
    const size_t lds_bytes = (size_t)W::kI8Slots * W::kI8SbPerSlot * kI8SbLds;
    for (auto pass : passes)
        if (int rc = ensure_dynamic_lds((const void*)pass, (int)lds_bytes)) return rc;
    const char* q8 = ws + p.off_q8;
    const f32x4* qab = (const f32x4*)(ws + p.off_qab);
    const float* qlam = (const float*)(ws + p.off_qlam);
    unsigned* gmax = (unsigned*)(ws + p.off_gmax);
    u64 *scand = (u64*)(ws + p.off_scand), *gstar = (u64*)(ws + p.off_gstar), *best = (u64*)(ws + p.off_best);
    int *wave_cnt = (int*)(ws + p.off_sctl) + 64, *ctl8 = (int*)(ws + p.off_ctl8);
    const int n_sb = (int)((h->ntotal + 31) / 32), G8 = W::i8_grid(p);
    for (int gi = 0; gi < group_count(W::kQ, nq); ++gi) {
        const QGroup g = query_group(W::kQ, nq, gi, 1);
        const size_t g0 = (size_t)g.q0;
        if (gi) MDR_HIP_TRY(hipMemsetAsync(ctl8 + 3, 0, sizeof(int), st));  // emitted-candidate total of this group's pass
        for (auto pass : passes) {
            hipLaunchKernelGGL(pass, dim3(G8), dim3(512), lds_bytes, st, (const char*)h->i8, (long long)h->ntotal, n_sb, q8 + g0 * h->d, qab + g0, g.n, g.q0,
                               gmax + g0, scand, wave_cnt, ctl8, gstar + g0, (const u64*)best, qlam + g0);
            hipLaunchKernelGGL(mips_star8_kernel, dim3((g.n + 15) / 16), dim3(256), 0, st, (const char*)h->hi, (const char*)h->lo, h->nkb,
                               q_dev + g0 * h->d, (const u64*)(gstar + g0), g.n, best + g0, row_unscale(h));
        }
        hipLaunchKernelGGL(mips_refine8_kernel, dim3(G8 * 8), dim3(256), 0, st, (const char*)h->hi, (const char*)h->lo, h->nkb, q_dev, (const u64*)scand,
                           (const int*)wave_cnt, (const unsigned*)gmax, best, ctl8, kI8RefinePerQuery * g.n, qab, row_unscale(h));
        MDR_HIP_TRY(hipGetLastError());
    }
    return MDR_OK;
}

template <class W, bool BF>
int ensure_screenk_lds() {
    const int rc = ensure_dynamic_lds((const void*)W::template screen<2, BF>(), (int)kScreenLds);
    return rc ? rc : ensure_dynamic_lds((const void*)W::template screenk<BF>(), (int)kScreenLds);
}

// one query group of the k > 1 screen on the kernels of width W: sample pass -> k-th of the workgroup maxima -> screen-k pass -> merge / refine.
// Query fragments, bounds, thresholds and outputs are linear in the query number for both widths; the per-query lists have stride W::kQ.
template <class W, bool BF>
int screenk_group(mdr_index* h, const SearchPlan& p, char* ws, const float* q_dev, QGroup g, int k, float* D_dev, long long* I_dev, long long id_offset,
                  hipStream_t st) {
    const size_t g0 = (size_t)g.q0;
    const char* qg = ws + p.off_qhi + g0 * h->d * 2;
    const float* bg = (const float*)(ws + p.off_bound) + g0;
    float* tg = (float*)(ws + p.off_gmax) + g0;
    unsigned* wgmax = (unsigned*)(ws + p.off_scand);
    int* sctl = (int*)(ws + p.off_sctl);
    u64* cand = (u64*)(ws + p.off_cand);
    int* cnt = (int*)(ws + p.off_cnt);
    const int n_sb = (int)((h->ntotal + 31) / 32), stages = sample_stages_for(k);
    MDR_HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)p.G * W::kQ * 4, st));
    MDR_HIP_TRY(hipMemsetAsync(wgmax, 0, (size_t)p.G * stages * W::kQ * 4, st));
    hipLaunchKernelGGL((W::template screen<2, BF>()), dim3(p.G), dim3(512), kScreenLds, st, (const char*)h->hi, (long long)h->ntotal, n_sb, qg, bg, g.n, g.q0,
                       wgmax, (u64*)nullptr, (int*)nullptr, (int*)nullptr, (const int*)nullptr, stages);
    hipLaunchKernelGGL(kth_of_maxima_kernel, dim3(g.n), dim3(256), 0, st, (const unsigned*)wgmax, p.G * stages, k, tg, W::kQ);
#if MDR_MIPS_GEMMK
    if (W::kQ == kWideQ && gemmk_runs(h, p))  // measurement build: the main pass as a 256 x 256 x 64 GEMM with the screen as its epilogue (mdr_mips_gemmk.inl)
        hipLaunchKernelGGL((mips_gemmk_kernel<BF>), dim3(p.G), dim3(512), kGemmkLds, st, (const char*)h->hi, (long long)h->ntotal, qg, bg, (const float*)tg, g.n,
                           cand, cnt, sctl);
    else
#endif
        hipLaunchKernelGGL((W::template screenk<BF>()), dim3(p.G), dim3(512), kScreenLds, st, (const char*)h->hi, (long long)h->ntotal, n_sb, qg, bg,
                           (const float*)tg, g.n, cand, cnt, k, sctl);
    hipLaunchKernelGGL((merge_screenk_kernel<BF>), dim3(g.n), dim3(256), kMergeKLdsBytes, st, (const u64*)cand, (const int*)cnt, p.G, k, bg, (const char*)h->hi,
                       (const char*)h->lo, h->nkb, q_dev + g0 * h->d, D_dev + g0 * k, I_dev + g0 * k, id_offset, sctl, W::kQ, row_unscale(h));
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

// 2 <= k <= 256 on the screen path; sctl[0] = overflow flag for the conditional exact pass. In a wide call a group of at most 128 queries goes through
// the 16-queries-per-wave kernels instead (round 4; nq = 800: 3 x 256 + 32): a pass of theirs is HBM-bound on the hi plane (1.6 ms at 5 M rows), a
// 32-queries-per-wave pass costs its MFMA skeleton whatever the number of queries (2.15 ms). Under the old cut that is the remainder group, under the
// even cut only mode 2 does it.
template <class W, bool BF>
int run_screenk(W, Flag<BF>, mdr_index* h, const SearchPlan& p, char* ws, const float* q_dev, int nq, int k, float* D_dev, long long* I_dev,
                long long id_offset, hipStream_t st) {
    int rc = ensure_screenk_lds<W, BF>();
    if (W::kQ == kWideQ) {  // a wide call may run the narrow kernels too (below) and, in a measurement build, the GEMM-structured pass
#if MDR_MIPS_GEMMK
        if (!rc) rc = ensure_dynamic_lds((const void*)mips_gemmk_kernel<BF>, (int)kGemmkLds);
#endif
        if (!rc) rc = ensure_screenk_lds<Narrow, BF>();
    }
    if (!rc) rc = ensure_dynamic_lds((const void*)merge_screenk_kernel<BF>, (int)kMergeKLdsBytes);
    if (rc) return rc;
    MDR_HIP_TRY(hipMemsetAsync(ws + p.off_sctl, 0, 256, st));
    const int ngroups = group_count(W::kQ, nq);
    for (int gi = 0; gi < ngroups && !rc; ++gi) {
        const QGroup g = query_group(W::kQ, nq, gi, k);
        const bool narrow = ngroups > 1 && g.n <= kStreamQ && (even_groups_mode() == 2 || (!even_cut(k) && gi == ngroups - 1));
        rc = narrow ? screenk_group<Narrow, BF>(h, p, ws, q_dev, g, k, D_dev, I_dev, id_offset, st)
                    : screenk_group<W, BF>(h, p, ws, q_dev, g, k, D_dev, I_dev, id_offset, st);
    }
    return rc;
}

// exact pass, k == 1 (F32X2H): the stream kernel's register argmax into `best`, per group of kStreamQ queries
int run_stream_top1(mdr_index* h, const SearchPlan& p, char* ws, int nq, const int* run_if, hipStream_t st) {
    if (int rc = ensure_dynamic_lds((const void*)mips_stream_kernel<kNkb, 0>, (int)(3 * kStageBytes))) return rc;
    const char *qhi = ws + p.off_qhi, *qlo = ws + p.off_qlo;
    const float* qscale = (const float*)(ws + p.off_qscale);
    u64* best = (u64*)(ws + p.off_best);
    const int n_rb = (int)((h->ntotal + 15) / 16);
    for (int gi = 0; gi < group_count(kStreamQ, nq); ++gi) {
        const QGroup g = query_group(kStreamQ, nq, gi, 1);
        const size_t qoff = (size_t)g.q0 * h->d * 2;
        hipLaunchKernelGGL((mips_stream_kernel<kNkb, 0>), dim3(p.Gx), dim3(512), 3 * kStageBytes, st, (const char*)h->hi, (const char*)h->lo, (long long)h->ntotal,
                           n_rb, qhi + qoff, qlo + qoff, g.n, best + g.q0, (u64*)nullptr, (int*)nullptr, (u64*)nullptr, 1, run_if, qscale + g.q0);
        MDR_HIP_TRY(hipGetLastError());
    }
    return MDR_OK;
}

// exact pass, 2 <= k <= 128 (F32X2H): the stream kernel with candidate lists + merge, per group of kStreamQ queries
int run_stream_topk(mdr_index* h, const SearchPlan& p, char* ws, int nq, int k, float* D_dev, long long* I_dev, long long id_offset, const int* run_if,
                    hipStream_t st) {
    const size_t lds_bytes = 3 * kStageBytes + kStreamQ * sizeof(int);
    if (int rc = ensure_dynamic_lds((const void*)mips_stream_kernel<kNkb, 1>, (int)lds_bytes)) return rc;
    const char *qhi = ws + p.off_qhi, *qlo = ws + p.off_qlo;
    const float* qscale = (const float*)(ws + p.off_qscale);
    u64* cand = (u64*)(ws + p.off_cand);
    int* cnt = (int*)(ws + p.off_cnt);
    u64* kth = (u64*)(ws + p.off_kth);
    const int n_rb = (int)((h->ntotal + 15) / 16);
    for (int gi = 0; gi < group_count(kStreamQ, nq); ++gi) {
        const QGroup g = query_group(kStreamQ, nq, gi, k);
        const size_t qoff = (size_t)g.q0 * h->d * 2;
        MDR_HIP_TRY(hipMemsetAsync(cnt, 0, (size_t)p.Gx * kStreamQ * 4, st));
        MDR_HIP_TRY(hipMemsetAsync(kth, 0, (size_t)p.Gx * kStreamQ * 8, st));
        hipLaunchKernelGGL((mips_stream_kernel<kNkb, 1>), dim3(p.Gx), dim3(512), lds_bytes, st, (const char*)h->hi, (const char*)h->lo, (long long)h->ntotal,
                           n_rb, qhi + qoff, qlo + qoff, g.n, (u64*)nullptr, cand, cnt, kth, k, run_if, qscale + g.q0);
        hipLaunchKernelGGL(merge_lists_kernel, dim3(g.n), dim3(256), 0, st, (const u64*)cand, (const int*)cnt, (const u64*)kth, p.Gx, kStreamQ, kStreamCap, k,
                           D_dev + (size_t)g.q0 * k, I_dev + (size_t)g.q0 * k, id_offset, run_if, qscale + g.q0);
        MDR_HIP_TRY(hipGetLastError());
    }
    return MDR_OK;
}
