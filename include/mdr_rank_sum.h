/*
 * include/mdr_rank_sum.h -- C ABI of the ordered gradient sum of multi-rank training in libmdrhip.so (gfx950). The conventions of
 * include/mdr_hip.h hold (int return codes, mdr_last_error(), device pointers, `stream` = hipStream_t as void*, caller-owned buffers,
 * enqueued on `stream` on the caller's current device, no synchronisation and no host readback).
 *
 * recv holds n_ranks rows of `stride` floats: row r is rank r's contribution to this rank's segment of the flat gradient buffer
 * (multihop_dense_retrieval_amd/dist.py). mdr_rank_sum writes
 *
 *     out[i] = (((recv[0 * stride + i] + recv[1 * stride + i]) + recv[2 * stride + i]) + ...)        for i < n
 *
 * in fp32, strictly left to right in rank order: no FMA, no reassociation, the accumulator starts at row 0 (not at 0), so n_ranks == 1 copies
 * the bits and -0.0 survives. The replay is numpy float32 adding one row after another (dist.rank_sum_host). Non-finite values follow IEEE
 * 754: +inf in one rank and -inf in another give NaN, which is how an fp16 overflow on one rank reaches every rank's optimizer. Elements
 * n .. stride - 1 of a row are never read into a result and nothing outside out[0 .. n) is written. No atomics: two calls give the same bits.
 *
 * Validated on the host without a launch, MDR_E_INVALID with mdr_last_error(): a NULL pointer, n_ranks outside 1 .. MDR_RANK_SUM_MAX_RANKS,
 * n < 1, stride < n, stride % 4 != 0, a pointer that is not 16-byte aligned, out[0 .. n) overlapping the rows of recv.
 */
#ifndef MDR_RANK_SUM_H
#define MDR_RANK_SUM_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_RANK_SUM_MAX_RANKS 16

int mdr_rank_sum(const float* recv, int n_ranks, int64_t n, int64_t stride, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_RANK_SUM_H */
