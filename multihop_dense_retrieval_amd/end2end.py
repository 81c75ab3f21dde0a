"""End-to-end HotpotQA QA (the reference's scripts/end2end.py): question -> two-hop retrieval -> top-k chains -> reader -> answer, on one
MI355X.

    python scripts/end2end.py hotpot_qas_val.json --indexpath wiki_index.npy --corpus_dict hotpotQA_corpus_dict.json \
        --retriever_path q_encoder.pt --reader_path qa_electra.pt --topk 20 --batch-size 100 --sp-pred --save-prediction out.json

Per batch of --batch-size questions: the retrieval loop of the eval CLI (pipeline.TwoHopPipeline with the hop-2 token arena, beam = topk)
and mhop.rank_paths on the host; the question's WordPieces once on the host; the batch shape from the QA arena's host metadata; the
reader rows assembled on the device from the chain ids (qa_arena.assemble, mdr_reader_assemble), then QAModel.decode() over all chains of
the batch (--reader-batch-size rows per forward); only start / end / rank / span / sp per chain come back. The answer of a question is
eval_final's: the first chain of the stable sort on 0.8 rank + 0.2 span; prepare() and the text decode run for that chain only.
Log lines, the printed lines and the --save-prediction JSON ({"answer", "sp", "titles"}) are the reference's.

Deliberate differences from the reference:
- Index format: --indexpath is the .npy matrix the eval CLI takes; a FAISS HNSW file is refused (exact search is the product).
- Path score: the exact inner product D + D' (the reference ranks by the HNSW index's negated distances).
- Empty hop-1 passage: its chains rank LAST, as in the eval CLI; the reference's `-(scores_1 + scores_2)` with scores_1 = -inf sends them first.
- Question count: every question is read (the reference keeps `readlines()[:5]`, a debugging leftover); --max-questions N caps it.
- Model names: `roberta-base` and `google/electra-large-discriminator` are loaded locally (local_files_only); --retriever-model and
  --reader-model override them. The reader's tokenizer is BertTokenizer, as in scripts/train_qa.py.
- Reader numerics: the reference runs its reader in fp32 on the CPU (`eval_final(..., gpu=False)`); here it is the HIP reader with
  apex-O1 numerics (reader.py), whose rank and span scores are fp16. eval_final's 0.8 rank + 0.2 span selection and the span argmax
  therefore work on fp16-rounded scores: where two chains or two spans are closer than that rounding plus the O1 logit error, the
  choice can differ from the reference's (tests/test_end2end_gpu.py states the margin).
- Device: one rank, device only, no CPU fallback. Retrieval of all questions runs first (the eval CLI's pipelined loop), then the
  reader walks the same batches; the outputs are those of the batch-by-batch order. "Loading corpus..." comes before "Loading index...":
  the corpus arenas are built before the process touches the device.
"""
import argparse
import json
import logging
import os
import time

import numpy as np
import torch

from . import mhop, qa_data

logger = logging.getLogger()

READER_MAX_SEQ_LEN, READER_MAX_Q_LEN = 512, 64  # QAEvalDataset(..., max_seq_len=512, max_q_len=64) in the reference


class RunResult(dict):
    """main()'s return value: the --save-prediction dict ({"answer", "sp", "titles"}), plus `chains` (per question [(hop-1 id, hop-2 id)] in rank
    order) and `seconds` (retrieval / assembly / reader / host decode)."""


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("raw_data", type=str, default=None)
    p.add_argument("--indexpath", type=str, default="retrieval/index/wiki_index_hnsw_roberta")
    p.add_argument("--corpus_dict", type=str, default="retrieval/index/hotpotQA_corpus_dict.json")
    p.add_argument("--retriever_path", type=str, default="")
    p.add_argument("--reader_path", type=str, default="")
    p.add_argument("--topk", type=int, default=1, help="topk paths")
    p.add_argument("--num-workers", type=int, default=10)
    p.add_argument("--max-q-len", type=int, default=70)
    p.add_argument("--max-q-sp-len", type=int, default=350)
    p.add_argument("--batch-size", type=int, default=1)
    p.add_argument("--max-ans-len", default=35, type=int)
    p.add_argument("--save-prediction", default="", type=str)
    p.add_argument("--model-name", type=str, default="")
    p.add_argument("--sp-pred", action="store_true", help="whether to predict sentence sp")
    p.add_argument("--sp-weight", default=0, type=float, help="weight of the sp loss")
    # extensions (not in the reference)
    p.add_argument("--max-questions", type=int, default=None, help="read only the first N questions (default: all)")
    p.add_argument("--retriever-model", type=str, default="roberta-base", help="local model directory or cached name of the retriever")
    p.add_argument("--reader-model", type=str, default="google/electra-large-discriminator", help="local model directory or cached name of the reader")
    p.add_argument("--reader-batch-size", type=int, default=0, help="chains per reader forward (default: all chains of a question batch)")
    p.add_argument("--qa-arena-workers", type=int, default=16, help="processes that tokenise the corpus for the reader on first use (at most 16)")
    return p


def _setup_logging():
    logger.setLevel(logging.INFO)
    if logger.hasHandlers():
        logger.handlers.clear()
    logger.addHandler(logging.StreamHandler())


def _hop2_arena(args, tokenizer, id2doc):
    from .arena import TokenArena, arena_tag
    cache = args.corpus_dict + ".arena.npz"
    tag = arena_tag(tokenizer, True, args.max_q_sp_len)
    arena = None
    if os.path.exists(cache):
        try:
            arena = TokenArena.load(cache, expect_tag=tag)
        except (OSError, ValueError, EOFError):
            arena = None
    if arena is None:
        logger.info("Tokenising the corpus once for device-side hop-2 assembly...")
        arena = TokenArena.from_corpus(id2doc, tokenizer, roberta=True, max_tokens=args.max_q_sp_len)
        arena.save(cache, tag=tag)
    return arena


def select_and_decode(batch_items, head, chains_psg, para_offsets, qa_tokenizer, sp_pred, weight=0.8):
    """eval_final for one question batch, decoding only the chosen chain of each question.
    batch_items: [{"_id", "question"}] (question as read); head: per-row python lists (start, end, span_score, rank_score, sp_prob or None),
    rows question-major (k per question); chains_psg: per question [[doc1, doc2], ...]; para_offsets: per question (question WordPieces + 2).
    -> [(qid, answer dict)]."""
    k = len(chains_psg[0]) if chains_psg else 0
    out = []
    for b, item in enumerate(batch_items):
        rows = list(range(b * k, (b + 1) * k))
        order = sorted(rows, key=lambda r: weight * head["rank_score"][r] + (1 - weight) * head["span_score"][r], reverse=True)
        r = order[0]
        q = item["question"][:-1] if item["question"].endswith("?") else item["question"]
        passages = chains_psg[b][r - b * k]
        prep = qa_data.prepare({"question": q, "passages": passages}, qa_tokenizer)
        ann = prep["context_processed"]
        po = para_offsets[b]
        wp = ann["all_doc_tokens"][:READER_MAX_SEQ_LEN - po - 1]
        batch = {"net_inputs": {"label": torch.tensor([[-1]])}, "qids": [item["_id"]], "para_offsets": [po], "passages": [passages],
                 "tok_to_orig_index": [ann["tok_to_orig_index"]], "doc_tokens": [ann["doc_tokens"]], "wp_tokens": [wp]}
        one = {"start": [head["start"][r]], "end": [head["end"][r]], "span_score": [head["span_score"][r]], "rank_score": [head["rank_score"][r]],
               "sp_prob": [head["sp_prob"][r]] if head["sp_prob"] is not None else None}
        (qid, _, ans), = qa_data.chain_results(batch, one, sp_pred, final=True)
        out.append((qid, ans))
    return out


def question_ids(qa_tokenizer, questions):
    """QAEvalDataset's question WordPieces (one trailing "?" stripped, cut to max_q_len) as ids: the only tokenisation of a question on the reader side."""
    from . import qa_arena
    return [qa_arena.question_ids(qa_tokenizer, q, READER_MAX_Q_LEN) for q in questions]


def assemble_batch(qa_arena_obj, special, q_ids, chains, device):
    """Reader rows of one question batch on the device. q_ids: question_ids() of the batch; chains: int [B, k, 2] passage ids.
    -> (dict of device tensors as qa_arena.assemble returns them, (out_len, n_sent))."""
    from . import qa_arena
    B = len(q_ids)
    ch = np.asarray(chains, np.int64).reshape(-1, 2)
    k = ch.shape[0] // max(1, B)
    row_q = np.repeat(np.arange(B, dtype=np.int64), k)
    L, S = qa_arena_obj.batch_shape([len(q) for q in q_ids], ch, row_q, READER_MAX_SEQ_LEN)
    qt = np.zeros((B, max(1, max(len(q) for q in q_ids))), np.int64)
    for b, q in enumerate(q_ids):
        qt[b, :len(q)] = q
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device, non_blocking=False)  # noqa: E731
    rows = qa_arena.assemble(qa_arena_obj, to(qt), to(np.asarray([len(q) for q in q_ids], np.int64)), to(ch), to(row_q), special,
                             READER_MAX_SEQ_LEN, L, S)
    return rows, (L, S)


def main(argv=None, retrieval_tokenizer=None, qa_tokenizer=None):
    args = build_parser().parse_args(argv)
    _setup_logging()
    if args.indexpath.endswith(".npy") is False or not os.path.isfile(args.indexpath):
        raise SystemExit(f"--indexpath {args.indexpath}: pass the .npy matrix of corpus embeddings (exact inner-product search); FAISS HNSW "
                         "index files are not supported")
    if args.topk < 1:
        raise SystemExit("--topk must be >= 1")
    import transformers

    from . import qa_arena, reader
    from .eval_mhop_retrieval import _load_config
    from .pipeline import TokenizerPool
    from .retriever import RobertaRetriever, load_saved

    logger.info("Loading trained models...")
    if retrieval_tokenizer is None:
        from .data import load_tokenizer
        retrieval_tokenizer = load_tokenizer(args.retriever_model)
    args.model_name = args.retriever_model
    retriever = RobertaRetriever(_load_config(args.retriever_model), args)
    retriever = load_saved(retriever, args.retriever_path, exact=True, map_location="cpu")
    qa_config = transformers.AutoConfig.from_pretrained(args.reader_model, local_files_only=True)
    if qa_tokenizer is None:
        qa_tokenizer = transformers.BertTokenizer.from_pretrained(args.reader_model, local_files_only=True)
    args.model_name = args.reader_model
    qa_model = reader.QAModel(qa_config, args)
    reader.load_saved(qa_model, args.reader_path, exact=False, map_location="cpu")

    logger.info("Loading corpus...")
    with open(args.corpus_dict) as f:
        id2doc = json.load(f)
    logger.info(f"Corpus size {len(id2doc)}")
    hop2_arena = _hop2_arena(args, retrieval_tokenizer, id2doc)
    qa_ar = qa_arena.QAArena.load_or_build(args.corpus_dict, id2doc, qa_tokenizer, workers=args.qa_arena_workers, log=logger.info)
    special = qa_arena.special_ids(qa_tokenizer)
    pool = TokenizerPool(retrieval_tokenizer, args.num_workers)  # forked before the device is touched
    try:
        return _run(args, retriever, qa_model, qa_tokenizer, id2doc, hop2_arena, qa_ar, special, pool)
    finally:
        pool.close()


def answer_line(results, id2gold_ans):
    """The reference's last log line, its np.mean over f1_score's (f1, precision, recall) tuples included."""
    ems = [qa_data.exact_match_score(results["answer"][q], id2gold_ans[q]) for q in results["answer"].keys()]
    f1s = [qa_data.f1_score(results["answer"][q], id2gold_ans[q]) for q in results["answer"].keys()]
    return f"Answer EM {np.mean(ems)}, F1 {np.mean(f1s)}"


def _run(args, retriever, qa_model, qa_tokenizer, id2doc, hop2_arena, qa_ar, special, pool):
    from .eval_mhop_retrieval import load_index
    from .pipeline import FinishPool, TwoHopPipeline
    device = torch.device("cuda", torch.cuda.current_device())
    logger.info("Loading index...")
    retriever.to(device)
    retriever.eval()
    qa_model.to(device).eval()
    index = load_index(args.indexpath, d=retriever.config.hidden_size)
    hop2_arena = hop2_arena.to(device)
    qa_ar.to(device)

    logger.info("Loading queries...")
    with open(args.raw_data) as f:
        qas_items = [json.loads(line) for line in f.readlines()]
    if args.max_questions is not None:
        qas_items = qas_items[:args.max_questions]
    questions = [mhop.strip_question(it["question"]) for it in qas_items]
    id2gold_ans = {it["_id"]: it["answer"][0] for it in qas_items}
    torch.cuda.synchronize()

    start = time.time()
    logger.info("Retrieving...")
    k = args.topk
    finish = lambda ann, D, I, D2, I2: mhop.rank_paths(D, I, D2, I2, k, k)  # noqa: E731
    finish_pool = FinishPool(finish, 0)
    pipe = TwoHopPipeline(retriever, index, pool, id2doc, finish, batch_size=args.batch_size, beam=k, max_q_len=args.max_q_len,
                          max_q_sp_len=args.max_q_sp_len, roberta=True, arena=hop2_arena, device=device, finish_pool=finish_pool)
    t0 = time.perf_counter()
    try:
        per_batch = [r for _, r in sorted(pipe.run(questions, qas_items), key=lambda t: t[0])]
    finally:
        pipe.close()
        finish_pool.close()
    torch.cuda.synchronize()
    t_retrieval = time.perf_counter() - t0
    ranked = [ch for r in per_batch for ch in r]  # per question [(h1, h2, score)] * k

    logger.info("Reading...")
    print(f"Total instances size {len(ranked) * k}")
    results = RunResult()
    for key in ("answer", "sp", "titles"):
        results[key] = {}
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t_asm = t_fwd = t_host = 0.0
    rbs = args.reader_batch_size if args.reader_batch_size > 0 else None
    for lo in range(0, len(qas_items), args.batch_size):
        items = qas_items[lo:lo + args.batch_size]
        chains = [[(h1, h2) for h1, h2, _ in ranked[lo + b]] for b in range(len(items))]
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        q_ids = question_ids(qa_tokenizer, [it["question"] for it in items])
        rows, _ = assemble_batch(qa_ar, special, q_ids, chains, device)
        e1.record()
        R = rows["input_ids"].shape[0]
        step = rbs or R
        heads = []
        for r0 in range(0, R, step):
            sub = {kk: rows[kk][r0:r0 + step] for kk in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets")}
            heads.append(qa_model.decode(sub, args.max_ans_len))
        e2.record()
        cat = lambda key: torch.cat([h[key].reshape(h[key].shape[0], -1) for h in heads])  # noqa: E731
        packed = torch.cat([cat("start").double(), cat("end").double(), cat("span_score").double(), cat("rank_score").double()], 1).cpu()
        sp = cat("sp_prob").float().cpu() if args.sp_pred and heads[0]["sp_prob"] is not None else None
        head = {"start": packed[:, 0].long().tolist(), "end": packed[:, 1].long().tolist(), "span_score": packed[:, 2].tolist(),
                "rank_score": packed[:, 3].tolist(), "sp_prob": sp.tolist() if sp is not None else None}
        t_asm += e0.elapsed_time(e1) / 1e3
        t_fwd += e1.elapsed_time(e2) / 1e3
        h0 = time.perf_counter()
        psg = [[[id2doc[str(a)], id2doc[str(c)]] for a, c in ch] for ch in chains]
        for qid, ans in select_and_decode(items, head, psg, [len(q) + 2 for q in q_ids], qa_tokenizer, args.sp_pred):
            results["answer"][qid] = ans["pred_str"]
            results["sp"][qid] = ans["pred_sp"]
            results["titles"][qid] = ans["chain_titles"]
        t_host += time.perf_counter() - h0
    if args.save_prediction != "":
        with open(args.save_prediction, "w") as f:
            json.dump(results, f)
    print(f"Finishing evaluation in {time.time() - start}s")

    logger.info(answer_line(results, id2gold_ans))
    results.chains = [[(int(h1), int(h2)) for h1, h2, _ in r] for r in ranked]
    results.seconds = {"retrieval": t_retrieval, "assembly": t_asm, "reader": t_fwd, "host_decode": t_host}
    return results


if __name__ == "__main__":
    main()
