// csrc/mdr_mhop_train.hip -- the retriever's training and dev batches assembled on the device from a token arena (include/mdr_mhop_train.h).
//
// Replaces, for scripts/train_mhop.py and scripts/train_momentum.py --do_train, the host work of MhopDataset.__getitem__ + mhop_collate on
// every sample of every batch of every epoch (six tokenizer calls a sample): the sequences are encoded once
// (multihop_dense_retrieval_amd/mhop_arena.py) and a step's twelve tensors are a gather of rows * 6 of them by a table of row ids.
// mhop_assemble_kernel is reader_train_assemble_kernel's (csrc/mdr_reader_train.hip) shape with the slot as the grid's second dimension:
// one 256-thread workgroup per (sample, slot), thread t writes positions t, t + 256, ... of that slot's output row, ids and mask, so each
// store instruction of a wave covers 64 consecutive int64 (512 contiguous bytes); the reads are the row's int32 tokens, contiguous too.
// Integer copies only. The six outputs have six widths: they come in one by-value table that is read with constant indices (pick), so the
// kernel keeps it in scalar registers.
// Bounds: every arena read sits behind `valid` (0 <= id < n_rows) and inside [offsets[id], offsets[id + 1]); every store is at a position
// < widths[slot] of sample < rows.
#include "../../include/mdr_mhop_train.h"
#include "mdr_common.h"

namespace mdr {
namespace {

constexpr int kMhopAssembleThreads = 256;
constexpr int kSlots = MDR_MHOP_SLOTS;

struct MhopOutputs {
    long long* ids[kSlots];
    long long* mask[kSlots];
    int width[kSlots];
};

// a[slot] for a workgroup-uniform slot without a dynamic index into the kernel's argument
template <typename T>
__device__ __forceinline__ T pick(const T (&a)[kSlots], int slot) {
    T v = a[0];
#pragma unroll
    for (int k = 1; k < kSlots; ++k) v = slot == k ? a[k] : v;
    return v;
}

__global__ void __launch_bounds__(kMhopAssembleThreads)
mhop_assemble_kernel(const int* __restrict__ a_tok, const long long* __restrict__ a_off, long long n_rows, const int* __restrict__ row_idx,
                     MhopOutputs out, int pad_id) {
    const int sample = blockIdx.x, slot = blockIdx.y, t = threadIdx.x;
    const int W = pick(out.width, slot);
    long long* ids = pick(out.ids, slot) + (size_t)sample * W;
    long long* msk = pick(out.mask, slot) + (size_t)sample * W;
    const long long r = row_idx[(size_t)sample * kSlots + slot];
    long long beg = 0;
    int n = 0;
    if (r >= 0 && r < n_rows) {
        beg = a_off[r];
        const long long len = a_off[r + 1] - beg;
        n = len < 0 ? 0 : (len > W ? W : (int)len);  // tokens of the row that are written
    }
    for (int p = t; p < W; p += kMhopAssembleThreads) {
        ids[p] = p < n ? (long long)a_tok[beg + p] : (long long)pad_id;
        msk[p] = p < n;
    }
}

}  // namespace
}  // namespace mdr

extern "C" int mdr_mhop_assemble(const mdr_mhop_arena* arena, const int32_t* row_idx_dev, int rows, const int32_t* widths, int64_t* const* ids,
                                 int64_t* const* mask, int pad_id, int device, void* stream) {
    using namespace mdr;
    const char* fn = "mdr_mhop_assemble";
    MDR_REQUIRE(rows >= 0, "%s: rows=%d", fn, rows);
    MDR_REQUIRE(arena && widths && ids && mask, "%s: NULL pointer", fn);
    MDR_REQUIRE(arena->n_rows >= 0, "%s: n_rows=%lld", fn, (long long)arena->n_rows);
    MDR_REQUIRE(arena->n_rows == 0 || (arena->tokens_dev && arena->offsets_dev), "%s: NULL arena array", fn);
    MhopOutputs out;
    for (int k = 0; k < kSlots; ++k) {
        MDR_REQUIRE(widths[k] >= 1, "%s: widths[%d]=%d", fn, k, (int)widths[k]);
        out.ids[k] = (long long*)ids[k];
        out.mask[k] = (long long*)mask[k];
        out.width[k] = widths[k];
    }
    if (rows == 0) return MDR_OK;
    MDR_REQUIRE(row_idx_dev, "%s: NULL row table", fn);
    for (int k = 0; k < kSlots; ++k) MDR_REQUIRE(out.ids[k] && out.mask[k], "%s: NULL output pointer (slot %d)", fn, k);
    MDR_ENTER_DEVICE(device);
    hipLaunchKernelGGL(mhop_assemble_kernel, dim3(rows, kSlots), dim3(kMhopAssembleThreads), 0, (hipStream_t)stream, (const int*)arena->tokens_dev,
                       (const long long*)arena->offsets_dev, (long long)arena->n_rows, (const int*)row_idx_dev, out, pad_id);
    MDR_HIP_TRY(hipGetLastError());
    return MDR_OK;
}
