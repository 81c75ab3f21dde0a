/*
 * include/mdr_reader.h -- C ABI of the HotpotQA answer reader in libmdrhip.so (gfx950).
 *
 * Replaces QAModel.forward at inference plus the span search of predict() / eval_final():
 *   mdr/qa/qa_model.py:27-109         ELECTRA (or BERT) encoder, qa_outputs, BertPooler + rank, sp
 *   scripts/train_qa.py:242-253       band-limited [B, L, L] span matrix and its two-stage max
 * The conventions of include/mdr_hip.h hold here (int return codes, mdr_last_error(), *_dev = device
 * pointers, `stream` = hipStream_t as void*, the caller owns every buffer it passes). The weight tensors use
 * the mdr_tensor type of that header.
 *
 * Numerics follow apex O1, the regime of the README's `--fp16` QA runs: fp16 GEMM operands with fp32
 * accumulation, LayerNorm / softmax / GELU in fp32, and every Linear of the heads returns fp16. The span
 * scores are fp16 sums (ties are common; the first (start, end) in row-major order wins, as torch's max does).
 */
#ifndef MDR_READER_H
#define MDR_READER_H

#include "mdr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdr_reader mdr_reader;

/* where the pooler dense layer (H x H, then tanh) lives in the checkpoint */
#define MDR_READER_POOLER_HEAD 0     /* "pooler.dense.*": QAModel's own BertPooler (ELECTRA checkpoints) */
#define MDR_READER_POOLER_ENCODER 1  /* "encoder.pooler.dense.*": the encoder's pooler (BERT-family checkpoints) */

typedef struct mdr_reader_config {
    int vocab, hidden, layers, heads, ffn, max_pos, type_vocab;
    float ln_eps;       /* 1e-12 for ELECTRA and BERT */
    int residual_fp32;  /* as mdr_encoder_config.residual_fp32; 2 = the apex-O1 dataflow */
    int has_sp;         /* 1: the checkpoint has sp.* (--sp-pred) */
    int pooler;         /* MDR_READER_POOLER_* */
} mdr_reader_config;

/* Copies the weights of the QAModel.state_dict() schema (encoder.embeddings.*, encoder.encoder.layer.{i}.*, the pooler,
 * qa_outputs.*, rank.*, sp.* when has_sp). Unknown names are ignored, a missing one is MDR_E_INVALID naming the key.
 * encoder.embeddings_project.* (ELECTRA-small, embedding size != hidden) is refused by name. */
int mdr_reader_create(const mdr_reader_config* cfg, const mdr_tensor* tensors, int n_tensors, int weights_on_device, int device,
                      void* stream, mdr_reader** out);
int mdr_reader_free(mdr_reader* h);

size_t mdr_reader_workspace_bytes(const mdr_reader* h, int batch, int seq_len, int n_sent);

/* Outputs of one forward; fp16 values are passed as their 16-bit patterns. Any pointer may be NULL to skip that output,
 * except start_logits / end_logits when the span search runs (span_start != NULL). */
typedef struct mdr_reader_outputs {
    uint16_t* start_logits;  /* fp16 [B, L]: -inf where paragraph_mask != 1 or mask == 0 */
    uint16_t* end_logits;    /* fp16 [B, L] */
    uint16_t* rank_score;    /* fp16 [B]: rank(tanh(pooler(h[:, 0]))) */
    uint16_t* sp_score;      /* fp16 [B, n_sent]: sp(h[b, sent_offsets[b, j]]), unmasked (QAModel's "sp_score") */
    uint16_t* sp_prob;       /* fp16 [B, n_sent]: sigmoid of sp_score, 0 where sent_offsets == 0 (predict()'s masked sigmoid) */
    int64_t* span_start;     /* [B]: argmax over s <= e <= s + max_ans_len of start[s] + end[e], first (s, e) among ties */
    int64_t* span_end;       /* [B] */
    uint16_t* span_score;    /* fp16 [B]: that maximum (-inf when every cell in the band is -inf; then (0, 0)) */
} mdr_reader_outputs;

/* ids / mask / token_type_ids / paragraph_mask: int64 [batch, seq_len], right-padded (mask 1 = token, 0 = pad, a prefix
 * of each row); token_type_ids may be NULL (all 0). sent_offsets: int64 [batch, n_sent] (may be NULL when n_sent == 0).
 * Padded positions are not computed: their logits are -inf (qa_collate gives them paragraph_mask 0), and an sp offset
 * that points past a row's tokens gets an sp_score of -inf. seq_len <= min(512, max_pos). */
int mdr_reader_forward(mdr_reader* h, const int64_t* ids_dev, const int64_t* mask_dev, const int64_t* token_type_ids_dev,
                       const int64_t* paragraph_mask_dev, const int64_t* sent_offsets_dev, int batch, int seq_len, int n_sent,
                       int max_ans_len, const mdr_reader_outputs* outputs, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The span search alone, on caller-given fp16 logits [batch, seq_len] (the same kernel mdr_reader_forward runs). */
int mdr_reader_span_search(const uint16_t* start_logits_dev, const uint16_t* end_logits_dev, int batch, int seq_len, int max_ans_len,
                           int64_t* span_start_dev, int64_t* span_end_dev, uint16_t* span_score_dev, int device, void* stream);

/* ---- reader input assembly from a QA passage arena (the end-to-end path) ----
 * Builds, for `rows` chains (passage ids p1, p2), the tensors qa_collate makes from QAEvalDataset items:
 *   input_ids       [CLS] q [SEP] wp [SEP] [PAD]...   wp = (yes no [SEP] P1 [SEP] P2) cut to max_seq_len - para_offset - 1
 *   attention_mask  1 on tokens; token_type_ids 1 on [para_offset, len); paragraph_mask 1 on [para_offset, len - 1)
 *   sent_offsets    [rows, n_sent]: the [unused1] positions of P1 then P2 inside the cut wp, + para_offset, zero-padded
 * with para_offset = q_len + 2 and len = para_offset + |wp| + 1. The arena holds each passage's WordPiece ids (tokens,
 * token_offsets [N + 1]) and its [unused1] positions relative to the passage (sent_starts, sent_offsets [N + 1]).
 * A passage id outside [0, N) is an empty passage and a question index outside [0, n_questions) an empty question.
 * Rows longer than out_len and sentences past n_sent are cut: the caller sizes both from the arena's host metadata. */
typedef struct mdr_reader_arena {
    const int32_t* tokens_dev;
    const int64_t* token_offsets_dev; /* [n_passages + 1] */
    const int32_t* sent_starts_dev;
    const int64_t* sent_offsets_dev;  /* [n_passages + 1] */
    int64_t n_passages;
} mdr_reader_arena;

typedef struct mdr_reader_batch {
    int64_t* input_ids;      /* [rows, out_len] */
    int64_t* attention_mask; /* [rows, out_len] */
    int64_t* token_type_ids; /* [rows, out_len] */
    int64_t* paragraph_mask; /* [rows, out_len]: qa_collate's float 0 / 1 as integers */
    int64_t* sent_offsets;   /* [rows, n_sent]; may be NULL when n_sent == 0 */
    int64_t* para_offsets;   /* [rows]; may be NULL */
    int64_t* lengths;        /* [rows]: len above, not clipped to out_len; may be NULL */
} mdr_reader_batch;

/* q_ids_dev int64 [n_questions, q_stride] (WordPiece ids, already cut to max_q_len), q_lens_dev int64 [n_questions],
 * chains_dev int64 [rows, 2], row_question_dev int64 [rows], special = {cls, sep, yes, no, pad} ids (host memory).
 * Requires max_seq_len - q_stride >= 6. One workgroup per row, integer copies only. */
int mdr_reader_assemble(const int64_t* q_ids_dev, const int64_t* q_lens_dev, int n_questions, int q_stride, const int64_t* chains_dev,
                        const int64_t* row_question_dev, int rows, const mdr_reader_arena* arena, const int32_t* special, int max_seq_len,
                        int out_len, int n_sent, const mdr_reader_batch* out, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MDR_READER_H */
