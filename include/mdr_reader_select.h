/*
 * include/mdr_reader_select.h -- C ABI of the reader's CHAIN SELECTION in libmdrhip.so (gfx950): which candidate chain of every question
 * predict() / eval_final() of scripts/train_qa.py read their answer from, for every combination factor at once, from the fp16 rank and
 * span scores of all chains (multihop_dense_retrieval_amd/qa_eval.py). The conventions of include/mdr_hip.h hold (int return codes,
 * mdr_last_error(), device pointers, `stream` = hipStream_t as void*, caller-owned buffers, enqueued on `stream`, no copy, no allocation,
 * no synchronisation and no host readback).
 *
 * The rule. predict() sorts a question's answer list IN PLACE, once per factor, with a stable descending sort on
 *     key_k(i) = fl(fl(lambda_k * rank_i) + fl(one_minus_k * span_i))          (Python floats: fp64, products and sum rounded separately)
 * so the sort for factor k starts from the order factor k - 1 left. The chain on top after factor k is therefore the one with the
 * lexicographically largest tuple (key_k, key_{k-1}, ..., key_0); among equal tuples the lowest index wins. winners[q, k] is that chain's
 * ITEM index (a position in rank16 / span16, not in the question). With one factor this is "first chain with the largest key".
 * Scores are fp16 bit patterns, widened exactly to fp64; comparisons are IEEE (-0.0 ties with 0.0); nothing is contracted into an FMA.
 * rank_top[q] is the first item with the largest rank score (the stable sort behind predict()'s "chain ranking em").
 *
 * Question q owns items q_offsets[q] .. q_offsets[q + 1] - 1. An empty question gets winners -1, rank_top -1, flags 0. A question with
 * any non-finite score (NaN, +inf, -inf: keys turn NaN, and a sort over NaN keys has no order a rule could state) gets flags 1,
 * winners -1 and rank_top -1: the caller runs the literal sort sequence on that question's scores. Every other question gets flags 0.
 * q_offsets is non-decreasing, starts at or above 0 and its last entry is below 2^31 and at most the length of the score arrays: the
 * caller guarantees it (the Python class checks it on the host, once).
 *
 * One wave of 64 lanes per question, four waves per workgroup, lanes striding over the question's items, one pass per factor and a
 * butterfly reduction under the same comparator; no LDS, no atomics: two runs give the same bits.
 *
 * Validated on the host without a launch, MDR_E_INVALID with mdr_last_error(): n_q < 0, n_lambda outside 1 .. MDR_READER_SELECT_MAX_LAMBDAS,
 * a NULL pointer (with n_q > 0). n_q == 0 is a no-op.
 */
#ifndef MDR_READER_SELECT_H
#define MDR_READER_SELECT_H

#include <stdint.h>

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_READER_SELECT_MAX_LAMBDAS 16

/* rank16_dev, span16_dev: fp16 bit patterns of every item; q_offsets_dev int64 [n_q + 1]; lambdas, one_minus: n_lambda doubles each in
 * HOST memory (one_minus[k] is the caller's 1 - lambdas[k], rounded as the caller rounds it); they travel as kernel arguments.
 * winners_dev int32 [n_q, n_lambda], rank_top_dev int32 [n_q], flags_dev int32 [n_q]. */
int mdr_reader_select(const uint16_t* rank16_dev, const uint16_t* span16_dev, const int64_t* q_offsets_dev, int n_q, const double* lambdas,
                      const double* one_minus, int n_lambda, int32_t* winners_dev, int32_t* rank_top_dev, int32_t* flags_dev, int device,
                      void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_READER_SELECT_H */
