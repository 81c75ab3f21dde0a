"""Measure ONE evaluation of scripts/train_qa.py (predict() over the eleven combination factors, as --do_train runs it) at ELECTRA-large
geometry (24 x 1024, 16 heads, FFN 4096) on a synthetic dev file, by the host path and by --eval-arena, on one device:

    python scripts/measure/qa_eval_bench.py [--questions 200] [--chains 50] [--predict_batch_size 128] [--rounds 2] [--out FILE.json]

The dev file has --questions questions with --chains candidate chains each, drawn as ordered pairs from a pool of 15 passages per question
(chains of one question share passages, as retrieved chains do); a chain's row is about 300 to 512 tokens, some cut at max_seq_len 512.
Its words are random words of the committed tiny vocabulary (tests/golden/reader_electra_tiny/vocab.txt: no real WordPiece vocabulary
travels with the tree; most words are one piece, which FLATTERS THE HOST PATH). The weights are random: the scores decide nothing here.

The two paths run in alternation, --rounds times each, every run in a child process of its own (this process never opens the device):
  host    QADataset + DataLoader + qa_collate, run_batches, qa_data.predict_metrics: the parent commit's path, the baseline
  arena   QAEvalPieces (built in the first arena run, loaded from its cache in the later ones), qa_eval.score_table,
          qa_eval.predict_metrics with mdr_reader_select
Each child reports its parts: host clocks around work that ends in a device synchronise, device events for the select kernel alone, and
(arena) qa_eval.select_sweep_host on the same scores. Both children print the metrics dict and a hash of the log lines; the parent checks
that they agree. Prints one JSON object; profiles/qa_eval.md holds a run."""
import argparse
import hashlib
import json
import logging
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

VOCAB = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny", "vocab.txt")
MAX_SEQ_LEN, MAX_Q_LEN, MAX_ANS_LEN, POOL = 512, 64, 35, 15


def write_dev_file(path, n_questions, n_chains, rng):
    words = [w for w in open(VOCAB).read().split("\n") if w.isalpha() and len(w) > 1 and w not in ("yes", "no")]

    def passage(title, n_tokens):
        sents, left = [], n_tokens
        while left > 0:
            k = min(left, rng.randint(12, 30))
            sents.append(" ".join(rng.choice(words) for _ in range(k - 1)) + " .")
            left -= k + 1  # the sentence marker
        return {"title": title, "sents": sents}

    with open(path, "w") as f:
        for q in range(n_questions):
            pool = [passage(f"p {q} {i}", rng.randint(140, 260)) for i in range(POOL)]
            pairs = rng.sample([(a, b) for a in range(POOL) for b in range(POOL) if a != b], n_chains)
            gold = pairs[rng.randrange(n_chains)]
            item = {"_id": f"d{q}", "question": " ".join(rng.choice(words) for _ in range(rng.randint(8, 20))) + " ?",
                    "answer": [" ".join(rng.choice(words) for _ in range(2))], "type": "bridge",
                    "sp": [dict(pool[i], sp_sent_ids=[0]) for i in gold], "candidate_chains": [[pool[a], pool[b]] for a, b in pairs]}
            f.write(json.dumps(item) + "\n")


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def child(a):
    import importlib.util
    import numpy as np
    import torch
    import transformers
    from functools import partial
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import qa_data, qa_eval, reader
    spec = importlib.util.spec_from_file_location("train_qa", os.path.join(ROOT, "scripts", "train_qa.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    logger = logging.getLogger("qa_eval_bench")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    lines = _Lines()
    logger.addHandler(lines)
    tok = transformers.BertTokenizer(VOCAB, do_lower_case=True)
    args = types.SimpleNamespace(model_name="google/electra-large-discriminator", sp_pred=True, max_ans_len=MAX_ANS_LEN)
    cfg = transformers.ElectraConfig(vocab_size=30522, hidden_size=1024, embedding_size=1024, num_hidden_layers=24, num_attention_heads=16,
                                     intermediate_size=4096, max_position_embeddings=512, type_vocab_size=2)
    res, clock = {"path": a.child}, time.perf_counter
    device = torch.device("cuda", 0)

    def synced(fn):
        torch.cuda.synchronize()
        t = clock()
        out = fn()
        torch.cuda.synchronize()
        return clock() - t, out

    pieces = None
    if a.child == "arena":  # before the device is opened: the builder's workers are forked
        cache = a.file + ".qa_eval_pieces.npz"
        res["cache"] = "load" if os.path.exists(cache) else "build"
        said = []
        t = clock()
        pieces = qa_eval.QAEvalPieces.load_or_build(a.file, tok, MAX_SEQ_LEN, MAX_Q_LEN, a.predict_batch_size, log=said.append, workers=a.workers)
        res["pieces_seconds"] = clock() - t
        t = clock()
        qa_eval.read_eval_file(a.file)
        res["of_which_reading_the_file"] = clock() - t
        res.update(items=pieces.n, questions=pieces.n_questions, distinct_passages=pieces.n_passages, cache_bytes=os.path.getsize(cache))
    model = reader.QAModel(cfg, args)
    g = torch.Generator().manual_seed(0)
    model.load_state_dict({k: 0.02 * torch.randn(shp, generator=g) for k, shp in model.state_dict().items()})
    model.to(device).eval()
    res["device"] = torch.cuda.get_device_name(0)
    if a.child == "host":
        t = clock()
        ds = qa_data.QADataset(tok, a.file, MAX_SEQ_LEN, MAX_Q_LEN)
        loader = DataLoader(ds, batch_size=a.predict_batch_size, collate_fn=partial(qa_data.qa_collate, pad_id=tok.pad_token_id), num_workers=0)
        res["dataset_seconds"] = clock() - t
        parts = {"items_and_collate": 0.0, "forward": 0.0}

        def timed_batches():
            it = iter(loader)
            while True:
                t0 = clock()
                try:
                    b = next(it)
                except StopIteration:
                    return
                parts["items_and_collate"] += clock() - t0
                yield b

        decode = model.decode

        def timed_decode(*x, **kw):
            dt, out = synced(lambda: decode(*x, **kw))
            parts["forward"] += dt
            return out

        model.decode = timed_decode
        total, (chains, gold) = synced(lambda: script.run_batches(model, timed_batches(), args, final=False))
        parts["read_back_and_decode_of_every_chain"] = total - parts["items_and_collate"] - parts["forward"]
        t = clock()
        metrics, _ = qa_data.predict_metrics(chains, gold, True, logger, fixed_thresh=None)
        parts["predict_metrics"] = clock() - t
        res["items"] = len(ds)
        res["evaluation_seconds"] = total + parts["predict_metrics"]
    else:
        res["to_device_seconds"], _ = synced(lambda: pieces.to(device))
        parts = {"assembly": 0.0, "forward": 0.0}
        table = qa_eval.ScoreTable(pieces.n, pieces.max_sents, device)
        t_all = clock()
        for lo, hi in pieces.batches:  # qa_eval.score_table, with a clock around its two halves
            dt, rows = synced(lambda: pieces.assemble(lo, hi))
            parts["assembly"] += dt
            dt, _ = synced(lambda: table.put(lo, model.decode({k: rows[k] for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask",
                                                                                   "sent_offsets", "label")}, MAX_ANS_LEN)))
            parts["forward"] += dt
        lambdas = qa_data.combination_factors(None)
        dt, w = synced(lambda: qa_eval.Winners(pieces, table, lambdas, tok, True, final=False))
        parts["select_read_back_and_decode_of_the_winners"] = dt
        t = clock()
        metrics, _ = qa_eval.predict_metrics(pieces, table, tok, True, logger, fixed_thresh=None)
        parts["predict_metrics_with_its_own_select_and_decode"] = clock() - t
        res["evaluation_seconds"] = clock() - t_all - dt  # (the Winners above are built again inside predict_metrics: counted once)
        per_q = [len(set(w.winners[j].tolist())) for j in range(len(w.winners)) if w.winners[j, 0] >= 0]
        res["winners"] = {"distinct": w.distinct, "per_question_mean": statistics.mean(per_q), "per_question_max": max(per_q), "flagged_questions": w.flagged}
        ev = []
        for _ in range(21):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            qa_eval.select(table.rank16, table.span16, pieces.dev["seg_offsets"], lambdas)
            e.record()
            torch.cuda.synchronize()
            ev.append(s.elapsed_time(e))
        res["select_kernel_ms"] = {"median": statistics.median(ev[1:]), "min": min(ev[1:]), "max": max(ev[1:])}
        r16, s16 = table.rank16.cpu().numpy(), table.span16.cpu().numpy()
        t = clock()
        sw, sr = qa_eval.select_sweep_host(r16, s16, pieces.seg_offsets, lambdas)
        res["select_sweep_host_ms"] = (clock() - t) * 1e3
        res["kernel_equals_sweep"] = bool(np.array_equal(sw, w.winners) and np.array_equal(sr, w.rank_top))
    res["parts_seconds"] = parts
    res["metrics"] = {k: float(v) for k, v in metrics.items()}
    res["log_sha256"] = hashlib.sha256("\n".join(lines.lines).encode()).hexdigest()
    res["log_lines"] = len(lines.lines)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=200)
    ap.add_argument("--chains", type=int, default=50)
    ap.add_argument("--predict_batch_size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--child-seconds", type=int, default=420, help="time limit of one child process")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="", choices=["", "host", "arena"])
    ap.add_argument("--file", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    tmp = tempfile.mkdtemp(prefix="qa_eval_bench_")
    dev_file = os.path.join(tmp, "dev.jsonl")
    write_dev_file(dev_file, a.questions, a.chains, random.Random(0))
    res = {"questions": a.questions, "chains_per_question": a.chains, "predict_batch_size": a.predict_batch_size, "dev_file_bytes": os.path.getsize(dev_file),
           "tokenizer": "the committed tiny vocabulary (132 entries): flatters the host path", "runs": []}
    for _ in range(a.rounds):
        for path in ("host", "arena"):  # alternated, each in a process of its own; a failed child ends the measurement
            cmd = [sys.executable, os.path.abspath(__file__), "--child", path, "--file", dev_file, "--predict_batch_size", str(a.predict_batch_size),
                   "--workers", str(a.workers)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_seconds)
            if r.returncode != 0:
                sys.exit(f"the {path} child ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            res["runs"].append(json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")][-1][7:]))
            print(f"[{path}] one evaluation: {res['runs'][-1]['evaluation_seconds']:.2f} s", file=sys.stderr, flush=True)
    res["paths_agree"] = len({(json.dumps(r["metrics"]), r["log_sha256"]) for r in res["runs"]}) == 1
    for path in ("host", "arena"):
        v = [r["evaluation_seconds"] for r in res["runs"] if r["path"] == path]
        res[path + "_evaluation_seconds"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
