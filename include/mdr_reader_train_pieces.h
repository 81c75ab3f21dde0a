/*
 * include/mdr_reader_train_pieces.h -- C ABI of the reader's TRAINING batch assembly from a PIECE arena in libmdrhip.so (gfx950): the
 * batches of scripts/train_qa.py --do_train --piece-arena, byte for byte those of mdr_reader_train_assemble (include/mdr_reader_train.h)
 * for the same item indices, spliced on the device from pieces that are stored once instead of from finished rows that repeat them.
 *
 * The candidate chains of one question share the question and most passages, and a chain's WordPieces are yes no [SEP] P1 [SEP] P2 with
 * each Pi a function of passage i alone (multihop_dense_retrieval_amd/qa_arena.py). The arena
 * (multihop_dense_retrieval_amd/qa_train_pieces.py) holds:
 *   q_tokens [sum lq] i32, q_offsets [Q + 1] i64         the question's WordPiece ids, already cut to max_q_len; one row per question
 *   p_tokens [sum lp] i32, p_offsets [P + 1] i64         one row per DISTINCT passage text, as include/mdr_reader.h's arena
 *   p_sent_starts [sum sp] i32, p_sent_offsets [P + 1] i64
 *                                                        the [unused1] positions relative to the passage, increasing, each < its length
 *   items [5 * N] i32                                    per item: question row, P1 row, P2 row, label, ans_covered
 *   sent_label [sum nl] i32, sent_label_index [N + 1] i64
 *                                                        the labels of the chain's sentences by ordinal (P1's, then P2's); an item holds
 *                                                        either none (they read as 0) or one per sentence of its chain
 *   spans [2 * sum np] i32, span_index [N + 1] i64       UNCUT (first, last) pairs in chain WordPiece positions (0 is `yes`); may be none
 * The index arrays are non-decreasing and end at their array's length and every row number of `items` lies inside its table: the caller
 * guarantees it (the Python class checks it on the host, once). max_q_len is the longest STORED question.
 *
 * mdr_reader_train_compose writes, for `rows` item indices, with po = len(q) + 2 and n_wp = min(3 + len(P1) + 1 + len(P2),
 * max(0, max_seq_len - po - 1)) (all int64):
 *   input_ids [rows, out_len]   [CLS] q [SEP] yes no [SEP] P1 [SEP] P2 cut to n_wp WordPieces, then [SEP], then special[4] (pad);
 *   attention_mask (1 on the po + n_wp + 1 tokens), token_type_ids (1 on [po, length)), paragraph_mask (1 on [po, length - 1));
 *   sent_offsets, sent_labels [rows, n_sent]   P1's starts + 3, then P2's starts + 4 + len(P1): those below n_wp, shifted by po, with the
 *                                               label of that ordinal (0 where the item holds none); 0 behind them;
 *   starts, ends [rows, n_span]   the item's pairs with first < n_wp, in stored order, compacted: first + po and
 *                                 min(last, n_wp - 1) + po; -1 behind them (so slot 0 is (-1, -1) when none is left);
 *   label, ans_covered [rows, 1]; para_offsets (po), lengths (po + n_wp + 1, not clipped to out_len) [rows] (optional: NULL skips).
 * An index outside [0, N) gives the EMPTY row of include/mdr_reader_train.h and reads nothing of the arena. Rows longer than out_len,
 * sentences past n_sent and spans past n_span are cut. n_sent == 0 takes NULL for sent_offsets and sent_labels.
 * One 256-thread workgroup per row, integer copies only, every store coalesced along the row; no atomics: two runs give the same bytes.
 */
#ifndef MDR_READER_TRAIN_PIECES_H
#define MDR_READER_TRAIN_PIECES_H

#include <stdint.h>

#include "mdr_reader_train.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdr_reader_train_pieces {
    const int32_t* q_tokens_dev;
    const int64_t* q_offsets_dev;        /* [n_questions + 1] */
    const int32_t* p_tokens_dev;
    const int64_t* p_offsets_dev;        /* [n_passages + 1] */
    const int32_t* p_sent_starts_dev;
    const int64_t* p_sent_offsets_dev;   /* [n_passages + 1] */
    const int32_t* items_dev;            /* [n_items, 5]: question row, P1 row, P2 row, label, ans_covered */
    const int32_t* sent_label_dev;
    const int64_t* sent_label_index_dev; /* [n_items + 1] */
    const int32_t* spans_dev;            /* (first, last) pairs */
    const int64_t* span_index_dev;       /* [n_items + 1], in pairs */
    int64_t n_items;
    int64_t n_questions;
    int64_t n_passages;
    int64_t max_q_len;                   /* the longest stored question */
} mdr_reader_train_pieces;

/* item_idx_dev int64 [rows]; special = {cls, sep, yes, no, pad} in HOST memory; out_len >= 1, n_sent >= 0, n_span >= 1,
 * max_seq_len - max_q_len >= 6 (room for yes no [SEP]); rows == 0 is a no-op. */
int mdr_reader_train_compose(const mdr_reader_train_pieces* arena, const int64_t* item_idx_dev, int rows, int max_seq_len, int out_len,
                             int n_sent, int n_span, const int32_t* special, const mdr_reader_train_batch* out, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_READER_TRAIN_PIECES_H */
