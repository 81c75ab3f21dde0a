/*
 * include/mdr_mhop_train.h -- C ABI of the retriever's TRAINING batch assembly in libmdrhip.so (gfx950): the six padded (ids, mask) pairs
 * of one mhop_collate batch (scripts/train_mhop.py and scripts/train_momentum.py --do_train, and their dev evaluations) built on the device
 * from a token arena, as mdr_reader_train_assemble (include/mdr_reader_train.h) builds the reader's batches from its item arena.
 *
 * The arena holds every encoded sequence the run can ask for (multihop_dense_retrieval_amd/mhop_arena.py: the questions, the distinct
 * passages and the question + start passage pairs, each tokenised ONCE and already cut) as
 *   tokens [sum len] i32, offsets [n_rows + 1] i64    row r is tokens[offsets[r] : offsets[r + 1]]
 * offsets is non-decreasing and ends at the token count: the caller guarantees it (the Python class checks it on the host).
 *
 * mdr_mhop_assemble takes a [rows, 6] table of arena row ids -- one line per sample, the slots in the order q, q_sp, c1, c2, neg1, neg2 --
 * and writes, for every slot k, ids[k] and mask[k], int64 [rows, widths[k]]: the row's tokens, then pad_id, and 1 on the tokens, then 0.
 * A row id outside [0, n_rows), negative ones included, gives an EMPTY row and reads nothing of the arena: pads and zeros. A row longer than
 * widths[k] is cut: the caller sizes the widths from the arena's host metadata.
 * ONE launch serves the twelve outputs: one 256-thread workgroup per (sample, slot), integer copies only, every store coalesced along the
 * row, offsets in 64-bit arithmetic; no atomics: two runs give the same bytes.
 * Returns MDR_OK, or MDR_E_INVALID (include/mdr_hip.h; the message behind mdr_last_error()) before anything is launched for a NULL arena,
 * table, widths or output pointer, rows < 0, n_rows < 0 or a width below 1.
 */
#ifndef MDR_MHOP_TRAIN_H
#define MDR_MHOP_TRAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDR_MHOP_SLOTS 6 /* q, q_sp, c1, c2, neg1, neg2 */

typedef struct mdr_mhop_arena {
    const int32_t* tokens_dev;
    const int64_t* offsets_dev; /* [n_rows + 1] */
    int64_t n_rows;
} mdr_mhop_arena;

/* row_idx_dev int32 [rows, 6]; widths[6] >= 1 (host); ids[k], mask[k] int64 [rows, widths[k]] (ids and mask: host arrays of six device
   pointers); rows == 0 is a no-op. */
int mdr_mhop_assemble(const mdr_mhop_arena* arena, const int32_t* row_idx_dev, int rows, const int32_t* widths, int64_t* const* ids,
                      int64_t* const* mask, int pad_id, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_MHOP_TRAIN_H */
