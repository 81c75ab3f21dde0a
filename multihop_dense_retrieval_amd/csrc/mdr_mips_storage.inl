// csrc/mdr_mips_storage.inl -- host side of the index's storage: growing the planes, converting added rows into them (exponent fit, fragment
// planes, int8 screening plane) and the pipelined upload of host-sourced rows. Included by mdr_mips.hip inside its unnamed namespace, after
// struct mdr_index and the kernel sections.

size_t plane_bytes_per_row(const mdr_index* h) { return (size_t)h->d * 2; }
float row_unscale(const mdr_index* h) { return ldexpf(1.f, h->xexp); }   // 2^E: stored rows -> the caller's scale
float row_scale_inv(const mdr_index* h) { return ldexpf(1.f, -h->xexp); }  // 2^-E
long long pad32(long long n) { return (n + 31) / 32 * 32; }

// the int8 screening plane exists for the storage / dimension the k = 1 screen path serves; MDR_MIPS_I8=0 (read at index creation) leaves it out
bool wants_i8(const mdr_index* h) {
    static const bool off = getenv("MDR_MIPS_I8") && atoi(getenv("MDR_MIPS_I8")) == 0;
    return !off && !h->compact && h->storage != MDR_STORE_BF16 && h->d == 768;
}

size_t elem_size(int dtype) { return dtype == MDR_DT_F32 ? 4 : 2; }
bool is_bf16(const mdr_index* h) { return h->storage == MDR_STORE_BF16; }

int grow(mdr_index* h, long long need_rows, hipStream_t st) {
    long long need = (need_rows + 255) / 256 * 256;  // whole 256-row tiles (mips_gemmk_kernel reads tiles; a multiple of 32 as every other kernel expects)
    if (need <= h->cap_rows) return MDR_OK;
    long long ncap = need;  // first reservation is exact; later ones grow by 1.5x
    if (h->cap_rows) {
        long long geo = (h->cap_rows + h->cap_rows / 2 + 255) / 256 * 256;
        if (geo > ncap) ncap = geo;
    }
    const size_t nbytes = (size_t)ncap * plane_bytes_per_row(h);
    const size_t used = (size_t)pad32(h->ntotal) * plane_bytes_per_row(h);
    char* planes[2] = {nullptr, nullptr};
    char* old[2] = {h->hi, h->lo};
    const int nplanes = h->storage == MDR_STORE_BF16 ? 1 : 2;
    for (int i = 0; i < nplanes; ++i) {
        MDR_HIP_TRY(hipMalloc((void**)&planes[i], nbytes));
        if (used) MDR_HIP_TRY(hipMemcpyAsync(planes[i], old[i], used, hipMemcpyDeviceToDevice, st));
        MDR_HIP_TRY(hipMemsetAsync(planes[i] + used, 0, nbytes - used, st));
    }
    char* n8 = nullptr;
    if (wants_i8(h) && !h->centre) {
        MDR_HIP_TRY(hipMalloc((void**)&h->centre, (size_t)h->d * 5 * 4));
        float init[3 * 1024];  // d <= 1024: c = 0, 1/w = 1, w = 1 until the first add() measures them
        for (int i = 0; i < 3 * h->d; ++i) init[i] = i < h->d ? 0.f : 1.f;
        MDR_HIP_TRY(hipMemcpy(h->centre, init, (size_t)h->d * 3 * 4, hipMemcpyHostToDevice));
    }
    if (wants_i8(h)) {
        const size_t sbb = i8_sb_bytes(h->d / 64), nb8 = (size_t)(ncap / 32 + 1) * sbb, used8 = (size_t)(pad32(h->ntotal) / 32) * sbb;  // + 1: the wide kernel's stages are super-block pairs
        MDR_HIP_TRY(hipMalloc((void**)&n8, nb8));
        if (used8) MDR_HIP_TRY(hipMemcpyAsync(n8, h->i8, used8, hipMemcpyDeviceToDevice, st));
        MDR_HIP_TRY(hipMemsetAsync(n8 + used8, 0, nb8 - used8, st));
    }
    MDR_HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < nplanes; ++i)
        if (old[i]) MDR_HIP_TRY(hipFree(old[i]));
    if (h->i8) MDR_HIP_TRY(hipFree(h->i8));
    h->hi = planes[0];
    h->lo = planes[1];
    h->i8 = n8;
    h->cap_rows = ncap;
    return MDR_OK;
}

template <typename T>
int launch_convert(bool bf, const T* src_dev, long long n_valid, long long n_total, int d, long long row0, char* dst_hi, char* dst_lo, int* flags,
                   float xinv, hipStream_t st) {
    long long threads = n_total * (d / 8);
    if (threads == 0) return MDR_OK;
    long long blocks = (threads + 255) / 256;
    if (bf)
        hipLaunchKernelGGL((convert_to_frag_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, st, src_dev, n_valid, n_total, d, row0, dst_hi, dst_lo, flags, 1.0f);
    else
        hipLaunchKernelGGL((convert_to_frag_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, st, src_dev, n_valid, n_total, d, row0, dst_hi, dst_lo, flags, xinv);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

constexpr long long kCentreRows = 65536;  // rows of the first add() the int8 plane's centre is averaged over

template <typename T>
int launch_add(mdr_index* h, const T* src_dev, long long n, long long row0, hipStream_t st) {
    const float xinv = h->storage == MDR_STORE_BF16 ? 1.0f : row_scale_inv(h);
    int rc = launch_convert(h->storage == MDR_STORE_BF16, src_dev, n, n, h->d, row0, h->hi, h->lo, h->flags, xinv, st);
    if (rc) return rc;
    hipLaunchKernelGGL(row_norm2_max_kernel<T>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, src_dev, n, h->d, h->flags, xinv);
    if (h->i8 && n > 0) {
        if (!h->centre_set) {  // the first rows this index ever sees define the centre of its int8 plane (any fixed vector is correct)
            const long long nc = n < kCentreRows ? n : kCentreRows;
            float* sums = h->centre + 3 * (size_t)h->d;
            MDR_HIP_TRY(hipMemsetAsync(sums, 0, (size_t)h->d * 8, st));
            const unsigned gy = (unsigned)((nc + 3) / 4 < 256 ? (nc + 3) / 4 : 256);
            hipLaunchKernelGGL(col_sum_kernel<T>, dim3((unsigned)((h->d + 63) / 64), gy), dim3(256), 0, st, src_dev, nc, h->d, sums);
            hipLaunchKernelGGL(centre_finish_kernel, dim3(1), dim3(1024), 0, st, (const float*)sums, h->d, 1.0f / (float)nc, h->centre, h->flags + 11);
            h->centre_set = true;
        }
        const long long want = (n + 3) / 4, cap = (long long)h->num_cus * 32;  // a wave walks rows r, r + 4 * grid, ...: centre and weights stay in registers
        hipLaunchKernelGGL(convert_to_i8_kernel<T>, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, src_dev, n, h->d, row0, h->i8, h->flags + 8,
                           (const float*)h->centre);
    }
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}

__global__ void scale_flag_float_kernel(int* __restrict__ flag, float f) { *flag = __float_as_int(__int_as_float(*flag) * f); }

// Fit the index exponent E (planes hold x * 2^-E) to the rows about to be converted; rows [0, row0) are already stored. Synchronises.
template <typename T>
int fit_exponent(mdr_index* h, const T* src_dev, long long n, long long row0, hipStream_t st) {
    if (h->storage == MDR_STORE_BF16 || n == 0) return MDR_OK;
    MDR_HIP_TRY(hipMemsetAsync(h->flags + 4, 0, sizeof(int), st));
    const long long count = n * (long long)h->d;
    const unsigned blocks = (unsigned)((count + 255) / 256 < 2048 ? (count + 255) / 256 : 2048);
    hipLaunchKernelGGL(absmax_kernel<T>, dim3(blocks), dim3(256), 0, st, src_dev, count, h->flags);
    MDR_HIP_TRY(hipGetLastError());
    int bits = 0;
    MDR_HIP_TRY(hipMemcpyAsync(&bits, h->flags + 4, sizeof(int), hipMemcpyDeviceToHost, st));
    MDR_HIP_TRY(hipStreamSynchronize(st));
    float m;
    memcpy(&m, &bits, 4);
    if (!(m <= 3.0e38f)) return set_error(MDR_E_RANGE, "add(): a value is non-finite; rows were not added");
    if (m == 0.f) return MDR_OK;
    int e = 0;
    (void)frexpf(m, &e);           // m in [2^(e-1), 2^e)
    const int target = e - 10;     // m * 2^-target in [2^9, 2^10): headroom of 2^5 before fp16 overflows
    if (!h->xexp_set) {
        h->xexp = target;
        h->xexp_set = true;
        return MDR_OK;
    }
    if (e - h->xexp > 15) {        // m * 2^-E >= 2^15 would not fit: grow E and shrink what is stored by the same power of two (exact)
        const float f = ldexpf(1.f, h->xexp - target);
        const long long n_vec8 = (row0 + 15) / 16 * 16 * (long long)h->d / 8;
        if (n_vec8 > 0) {
            hipLaunchKernelGGL(rescale_planes_kernel, dim3((unsigned)((n_vec8 + 255) / 256)), dim3(256), 0, st, h->hi, h->lo, n_vec8, f);
            hipLaunchKernelGGL(scale_flag_float_kernel, dim3(1), dim3(1), 0, st, h->flags + 2, f * f);  // max row |x|^2 in stored units
            MDR_HIP_TRY(hipGetLastError());
        }
        h->xexp = target;
    }
    return MDR_OK;
}

int add_any(mdr_index* h, const void* src_dev, int dtype, long long n, long long row0, hipStream_t st) {
    int rc = MDR_OK;
    switch (dtype) {  // (before anything is written: a non-finite value rejects the rows here)
        case MDR_DT_F32: rc = fit_exponent(h, (const float*)src_dev, n, row0, st); break;
        case MDR_DT_BF16: rc = fit_exponent(h, (const unsigned short*)src_dev, n, row0, st); break;
        case MDR_DT_F16: rc = fit_exponent(h, (const _Float16*)src_dev, n, row0, st); break;
        default: break;
    }
    if (rc) return rc;
    switch (dtype) {
        case MDR_DT_F32: return launch_add(h, (const float*)src_dev, n, row0, st);
        case MDR_DT_BF16: return launch_add(h, (const unsigned short*)src_dev, n, row0, st);
        case MDR_DT_F16: return launch_add(h, (const _Float16*)src_dev, n, row0, st);
        default: return set_error(MDR_E_INVALID, "unknown src_dtype %d", dtype);
    }
}

// threads of parallel_copy: MDR_UPLOAD_THREADS, else half the hardware threads up to 8
int upload_threads() {
    const unsigned hc = std::thread::hardware_concurrency();
    const char* env = getenv("MDR_UPLOAD_THREADS");
    return env ? (atoi(env) > 0 ? atoi(env) : 1) : (hc >= 16 ? 8 : hc >= 4 ? (int)hc / 2 : 1);
}

// memcpy with `nt` threads (page-cache / mmap sources fault their pages in here, in parallel)
void parallel_copy(char* dst, const char* src, size_t bytes, int nt) {
    if (nt <= 1 || bytes < (8u << 20)) { memcpy(dst, src, bytes); return; }
    std::vector<std::thread> th;
    const size_t part = (bytes / (size_t)nt + 4095) & ~(size_t)4095;
    size_t done_to = part < bytes ? part : bytes;  // [0, part) is this thread's; a part whose thread cannot be started (resource limits) is copied here too
    for (int t = 1; t < nt; ++t) {
        const size_t lo = (size_t)t * part;
        if (lo >= bytes) break;
        const size_t len = bytes - lo < part ? bytes - lo : part;
        try {
            th.emplace_back([=] { memcpy(dst + lo, src + lo, len); });
        } catch (...) {  // std::system_error: no more threads -- nothing may throw across the C ABI
            memcpy(dst + lo, src + lo, len);
        }
    }
    memcpy(dst, src, done_to);
    for (auto& t : th) t.join();
}

// Host-sourced rows (pageable memory, np.load(mmap_mode="r") included) -> the shard, as a two-slot pipeline (round 5; VERDICT r4 item 8: the 256 MiB
// copy -> convert -> sync series took ~2 s of a 5.6 s process for a 15.4 GB index):
//   producer thread   rows -> pinned slot (parallel memcpy) -> hipMemcpyAsync to the slot's device half on the COPY stream -> "copied" event
//   calling thread    waits for "copied" on `st`, runs add_any (range fit + conversion kernels, as before), records "converted"
// so chunk c + 1 is read from the host and crosses PCIe while chunk c is converted; a slot is refilled when its "converted" event has completed.
// Returns an error code (the caller rolls the index back); `n` rows starting at logical row h->ntotal.
int upload_host_rows(mdr_index* h, const char* rows, long long n, int src_dtype, size_t row_src, hipStream_t st) {
    // Slots are sized by the call (a 100-row add used to allocate 2 x 96 MiB of device staging + 2 x 96 MiB of pinned host memory and start a thread):
    // chunk = min(n, 96 MiB / row) rows, and an add that fits ONE small chunk takes the plain road -- one hipMemcpyAsync out of the caller's (pageable) rows into a
    // staging buffer of exactly that size, the conversion, a sync; no pinned memory, no producer thread.
    const size_t chunk_bytes_target = 96ull << 20, plain_bytes_max = 16ull << 20;
    long long chunk_rows = (long long)(chunk_bytes_target / row_src) > 0 ? (long long)(chunk_bytes_target / row_src) : 1;
    if (n < chunk_rows) chunk_rows = n;
    const size_t chunk_bytes = (size_t)chunk_rows * row_src;
    const long long nchunks = (n + chunk_rows - 1) / chunk_rows;
    const bool plain = nchunks == 1 && chunk_bytes <= plain_bytes_max;
    const size_t stage_need = plain ? chunk_bytes : 2 * chunk_bytes;
    if (stage_need > h->stage_bytes) {
        if (h->stage) MDR_HIP_TRY(hipFree(h->stage));
        h->stage = nullptr;
        h->stage_bytes = 0;
        MDR_HIP_TRY(hipMalloc(&h->stage, stage_need));
        h->stage_bytes = stage_need;
    }
    if (plain) {
        MDR_HIP_TRY(hipMemcpyAsync(h->stage, rows, chunk_bytes, hipMemcpyHostToDevice, st));
        int rc_p = add_any(h, h->stage, src_dtype, n, h->ntotal, st);
        if (rc_p == MDR_OK && hipStreamSynchronize(st) != hipSuccess) rc_p = set_error(MDR_E_HIP, "stream sync failed in add()");
        return rc_p;
    }
    if (chunk_bytes > h->pin_bytes) {
        for (int i = 0; i < 2; ++i) {
            if (h->pin[i]) MDR_HIP_TRY(hipHostFree(h->pin[i]));
            h->pin[i] = nullptr;
        }
        h->pin_bytes = 0;
        for (int i = 0; i < 2; ++i) MDR_HIP_TRY(hipHostMalloc(&h->pin[i], chunk_bytes, hipHostMallocDefault));
        h->pin_bytes = chunk_bytes;
    }
    if (!h->copy_st) MDR_HIP_TRY(hipStreamCreateWithFlags(&h->copy_st, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        if (!h->ev_copy[i]) MDR_HIP_TRY(hipEventCreateWithFlags(&h->ev_copy[i], hipEventDisableTiming));
        if (!h->ev_done[i]) MDR_HIP_TRY(hipEventCreateWithFlags(&h->ev_done[i], hipEventDisableTiming));
    }
    const int nt = upload_threads();
    struct Rows { long long r0, nr; };
    auto chunk = [&](long long c) { return Rows{c * chunk_rows, n - c * chunk_rows < chunk_rows ? n - c * chunk_rows : chunk_rows}; };  // rows of chunk c

    std::mutex mu;
    std::condition_variable cv;
    long long copied = 0, converted = 0;  // chunks whose H2D copy has been ISSUED / whose conversion has been ISSUED (its event recorded)
    bool abort_flag = false;
    int producer_rc = MDR_OK;
    const int device = h->device;
    auto produce = [&] {
        if (hipSetDevice(device) != hipSuccess) { std::lock_guard<std::mutex> g(mu); producer_rc = MDR_E_HIP; abort_flag = true; cv.notify_all(); return; }
        for (long long c = 0; c < nchunks; ++c) {
            const int slot = (int)(c & 1);
            if (c >= 2) {  // the slot's previous tenant (chunk c - 2) must have been converted: wait until that was issued, then until it completed
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return converted >= c - 1 || abort_flag; });
                if (abort_flag) return;
                lk.unlock();
                if (hipEventSynchronize(h->ev_done[slot]) != hipSuccess) { std::lock_guard<std::mutex> g(mu); producer_rc = MDR_E_HIP; abort_flag = true; cv.notify_all(); return; }
            }
            const auto [r0, nr] = chunk(c);
            parallel_copy((char*)h->pin[slot], rows + (size_t)r0 * row_src, (size_t)nr * row_src, nt);
            bool ok = hipMemcpyAsync((char*)h->stage + (size_t)slot * chunk_bytes, h->pin[slot], (size_t)nr * row_src, hipMemcpyHostToDevice, h->copy_st) == hipSuccess;
            ok = ok && hipEventRecord(h->ev_copy[slot], h->copy_st) == hipSuccess;
            std::lock_guard<std::mutex> g(mu);
            if (!ok) { producer_rc = MDR_E_HIP; abort_flag = true; cv.notify_all(); return; }
            if (abort_flag) return;
            copied = c + 1;
            cv.notify_all();
        }
    };
    std::thread producer;
    try {
        producer = std::thread(produce);
    } catch (...) {  // no thread to be had: the same chunks, one after the other, on this thread (nothing may throw across the C ABI)
        int rc_s = MDR_OK;
        for (long long c = 0; c < nchunks && rc_s == MDR_OK; ++c) {
            const auto [r0, nr] = chunk(c);
            memcpy(h->pin[0], rows + (size_t)r0 * row_src, (size_t)nr * row_src);
            if (hipMemcpyAsync(h->stage, h->pin[0], (size_t)nr * row_src, hipMemcpyHostToDevice, st) != hipSuccess) { rc_s = set_error(MDR_E_HIP, "hipMemcpyAsync(host rows) failed"); break; }
            rc_s = add_any(h, h->stage, src_dtype, nr, h->ntotal + r0, st);
            if (rc_s == MDR_OK && hipStreamSynchronize(st) != hipSuccess) rc_s = set_error(MDR_E_HIP, "stream sync failed in add()");
        }
        return rc_s;
    }
    int rc = MDR_OK;
    for (long long c = 0; c < nchunks && rc == MDR_OK; ++c) {
        const int slot = (int)(c & 1);
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return copied > c || abort_flag; });
            if (abort_flag) { rc = producer_rc ? set_error(producer_rc, "host upload pipeline failed (copy side)") : MDR_E_HIP; break; }
        }
        const auto [r0, nr] = chunk(c);
        if (hipStreamWaitEvent(st, h->ev_copy[slot], 0) != hipSuccess) { rc = set_error(MDR_E_HIP, "hipStreamWaitEvent failed in add()"); break; }
        rc = add_any(h, (char*)h->stage + (size_t)slot * chunk_bytes, src_dtype, nr, h->ntotal + r0, st);
        if (rc == MDR_OK && hipEventRecord(h->ev_done[slot], st) != hipSuccess) rc = set_error(MDR_E_HIP, "hipEventRecord failed in add()");
        std::lock_guard<std::mutex> g(mu);
        if (rc == MDR_OK) converted = c + 1;
        else abort_flag = true;
        cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> g(mu);
        if (rc != MDR_OK) abort_flag = true;
        cv.notify_all();
    }
    producer.join();
    (void)hipStreamSynchronize(h->copy_st);  // nothing of the caller's buffer or the pinned slots is in flight after return
    if (rc == MDR_OK && hipStreamSynchronize(st) != hipSuccess) rc = set_error(MDR_E_HIP, "stream sync failed in add()");
    return rc;
}
