"""Time the reader's training step and its --eval-arena evaluation on 1, 2 and 4 ranks and write profiles/reader_multirank.md:

    python scripts/measure/reader_multirank_bench.py [--out profiles/reader_multirank.md] [--steps 3] [--ranks 1,2,4] [--rounds 2]
        [--parent PATH]      # another checkout (the parent commit, built): its one-rank rows are measured in alternation with this one's

ELECTRA-large geometry with random weights, dropout 0.1, --sp-pred, the dynamic loss scale; a step of 12 rows padded to 512 tokens (lengths
uniform in [256, 512], two positives with a span, ten negatives, eight sentences a row), and one evaluation of the synthetic dev file of
scripts/measure/qa_eval_bench.py (--questions x --chains chains, --predict_batch_size 128) from its pieces. N ranks are N child processes
started here with RANK / WORLD_SIZE / LOCAL_RANK on a loopback address, each under a time limit; the first failure stops the run. With at
least N visible devices every rank has its own and the transport is nccl (RCCL); with fewer, all ranks share device 0 over gloo: the
rehearsal, in which the ranks queue behind each other on one card and the flat gradient buffer and the score rows cross the host, so such a
row says what the rehearsal costs, not what N devices would give. The profile says which rows are which.

Host clocks around work that ends in a device synchronise, rank 0's medians of --steps steps after one warm-up step. The step: this rank's
forward, backward and the ordered sum of the partial losses (train_step), then exchange, mdr_rank_sum, publish and the optimizer step;
`whole` is train_step + reduce() + opt.step() with one synchronise at the end. The evaluation: the decode of this rank's batches, the
merge (gather_objects + gather_rows + the fresh table), and predict_metrics (select, read-back, prepare() on the distinct winners, the
metrics), which every rank runs in full. The one-rank rows take no world: the code path of a run without a launcher.
"""
import argparse
import json
import logging
import os
import random
import socket
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD_LIMIT_S = 540
B, L, NS = 12, 512, 8


def median(v):
    return sorted(v)[len(v) // 2]


def make_batch(vocab):
    import numpy as np
    import torch
    rng = np.random.default_rng(12)
    lens = rng.integers(L // 2, L + 1, size=B)
    pos = np.arange(L)[None, :]
    mask = (pos < lens[:, None]).astype(np.int64)
    ids = np.where(mask == 1, rng.integers(1000, vocab, size=(B, L)), 0)
    po = 24  # question, yes / no and the separators in front of the passages
    label = np.zeros((B, 1), np.int64)
    label[::6] = 1
    starts = np.where(label == 1, rng.integers(po, L // 2 - 8, size=(B, 1)), -1)
    sent = np.sort(rng.integers(po, L // 2 - 1, size=(B, NS)), axis=1)
    net = {"input_ids": ids, "attention_mask": mask, "token_type_ids": ((pos >= po) & (mask == 1)).astype(np.int64),
           "paragraph_mask": ((pos >= po) & (pos < lens[:, None] - 1)).astype(np.int64), "label": label, "sent_offsets": sent,
           "sent_labels": rng.integers(0, 2, size=(B, NS)), "starts": starts, "ends": np.where(starts >= 0, starts + 3, -1)}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in net.items()}


def child(a):
    """One rank. `a.root` is the checkout whose package is measured."""
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(ROOT, "scripts", "measure"))
    import torch
    import transformers
    import qa_eval_bench as dev
    from multihop_dense_retrieval_amd import qa_eval, reader_train
    rank, N = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    world = bucket = None
    if N > 1:  # joined before anything opens the device, as the script does
        from datetime import timedelta
        import torch.distributed
        from multihop_dense_retrieval_amd import dist
        torch.distributed.init_process_group("gloo" if a.share_gpu else "nccl", timeout=timedelta(seconds=CHILD_LIMIT_S))
        world = dist.TorchWorld()
    tok = transformers.BertTokenizer(dev.VOCAB, do_lower_case=True)
    pieces = qa_eval.QAEvalPieces.load_or_build(a.file, tok, dev.MAX_SEQ_LEN, dev.MAX_Q_LEN, 128, workers=0)  # (the parent started from this cache too)
    torch.cuda.set_device(0 if a.share_gpu else int(os.environ.get("LOCAL_RANK", "0")))
    torch.manual_seed(0)  # the same weights on every rank
    cfg = transformers.ElectraConfig(vocab_size=30522, hidden_size=1024, embedding_size=1024, num_hidden_layers=a.layers, num_attention_heads=16,
                                     intermediate_size=4096, max_position_embeddings=512, type_vocab_size=2, hidden_dropout_prob=0.1,
                                     attention_probs_dropout_prob=0.1)
    args = types.SimpleNamespace(model_name="google/electra-large-discriminator", sp_pred=True, sp_weight=0.05, learning_rate=5e-5, adam_epsilon=1e-8,
                                 max_grad_norm=2.0, weight_decay=0.0, gradient_accumulation_steps=1, use_adam=False, fp16=True)
    model = reader_train.TrainableReader(cfg, args).cuda().train()
    opt = reader_train.optimizer_for(model, args)
    if world is not None:
        bucket = dist.GradBucket(model.parameters(), world)
    multi = {"world": world, "bucket": bucket} if world is not None else {}
    batch = make_batch(cfg.vocab_size)
    pieces.to(torch.device("cuda", torch.cuda.current_device()))
    sync, clock = torch.cuda.synchronize, time.perf_counter
    names = ("train_step", "exchange", "rank_sum", "publish", "optimizer", "whole")
    parts = {k: [] for k in names}
    for i in range(1 + a.steps):
        sync()
        t = [clock()]

        def mark():
            sync()
            t.append(clock())

        reader_train.train_step(model, batch, args, opt, 100 + i, **multi)
        mark()
        if world is None:
            mark(), mark(), mark()
        else:
            recv = world.exchange(bucket.flat)
            mark()
            dist.rank_sum(recv, bucket.mine)
            mark()
            world.publish(bucket.mine, bucket.flat)
            mark()
            del recv
        opt.step()
        mark()
        reader_train.train_step(model, batch, args, opt, 200 + i, **multi)
        if bucket is not None:
            bucket.reduce()
        opt.step()
        mark()
        if i >= 1:
            for k, d in zip(names, (t[j + 1] - t[j] for j in range(len(names)))):
                parts[k].append(d * 1e3)
    res = {"ranks": N, "transport": "none" if N == 1 else ("gloo, one shared device" if a.share_gpu else "nccl, a device per rank"),
           "step_ms": {k: median(v) for k, v in parts.items()}, "skipped_total": opt.read_state()["skipped_total"], "items": pieces.n,
           "questions": pieces.n_questions, "batches": len(pieces.batches)}
    logger = logging.getLogger("reader_multirank_bench")
    logger.addHandler(logging.NullHandler())
    logger.propagate = False
    ev = {"decode": [], "merge": [], "metrics": [], "whole": []}
    for i in range(1 + a.rounds):
        served = model.inference()
        sync()
        t0 = clock()
        if world is None:
            table = qa_eval.score_table(served, pieces, dev.MAX_ANS_LEN)
            sync()
            t1 = t2 = clock()
        else:
            first, behind = qa_eval.batch_deal(len(pieces.batches), N)[rank]
            local = qa_eval.ScoreTable(pieces.n, pieces.max_sents, pieces.dev["chains"].device)
            for lo, hi in pieces.batches[first:behind]:
                rows = pieces.assemble(lo, hi)
                local.put(lo, served.decode({k: rows[k] for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets", "label")},
                                            dev.MAX_ANS_LEN))
            sync()
            t1 = clock()
            table = qa_eval.merge_tables(local, pieces.batches, world)
            sync()
            t2 = clock()
        qa_eval.predict_metrics(pieces, table, tok, True, logger, fixed_thresh=None)
        t3 = clock()
        if i >= 1:
            for k, d in zip(("decode", "merge", "metrics", "whole"), (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                ev[k].append(d)
    res["eval_s"] = {k: median(v) for k, v in ev.items()}
    res["peak_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    if world is not None:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if rank == 0:
        print(json.dumps(res), flush=True)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(N, a, devices, root=ROOT):
    share = N > devices
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--steps", str(a.steps),
           "--rounds", str(a.rounds), "--layers", str(a.layers), "--file", a.file] + (["--share-gpu"] if share else [])
    port = free_port()
    children = [subprocess.Popen(cmd, stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, stderr=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True,
                                 env=dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(N), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)))
                for r in range(N)]
    out, err = children[0].communicate()
    codes = [c.wait() for c in children]
    if any(codes):
        print(f"{N} ranks: exit codes {codes}\n{err[-3000:]}", flush=True)
        sys.exit(1)  # the first failure stops the run: nothing more is started on the device
    r = json.loads(out.strip().split("\n")[-1])
    print(r, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reader_multirank.md"))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--ranks", default="1,2,4")
    ap.add_argument("--questions", type=int, default=40)
    ap.add_argument("--chains", type=int, default=50)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--dsplit", default=None, help="a text file with the d_split / d_perm table of tests/test_reader_multirank_step_gpu.py, appended verbatim")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--file", default="")
    ap.add_argument("--share-gpu", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    import tempfile
    import torch
    sys.path.insert(0, os.path.join(ROOT, "scripts", "measure"))
    import qa_eval_bench as dev
    devices = torch.cuda.device_count()
    tmp = tempfile.mkdtemp(prefix="reader_multirank_bench_")
    a.file = os.path.join(tmp, "dev.jsonl")
    dev.write_dev_file(a.file, a.questions, a.chains, random.Random(0))
    import transformers
    from multihop_dense_retrieval_amd import qa_eval
    qa_eval.QAEvalPieces.load_or_build(a.file, transformers.BertTokenizer(dev.VOCAB, do_lower_case=True), dev.MAX_SEQ_LEN, dev.MAX_Q_LEN, 128, workers=0)  # the cache, once
    one, parent = [], []
    for _ in range(2 if a.parent else 1):  # this checkout and the parent in alternation, one session
        one.append(run_ranks(1, a, devices))
        if a.parent:
            parent.append(run_ranks(1, a, devices, root=os.path.abspath(a.parent)))
    rows = [run_ranks(int(n), a, devices) for n in a.ranks.split(",") if int(n) > 1]
    r0 = one[0]
    lines = ["# The reader's training step and evaluation on several ranks", "",
             f"Command: `python scripts/measure/reader_multirank_bench.py --steps {a.steps} --rounds {a.rounds} --layers {a.layers} --ranks {a.ranks} --questions "
             f"{a.questions} --chains {a.chains}`{' --parent <the parent commit, built>' if a.parent else ''} ({devices} visible MI355X; ELECTRA-large geometry with "
             f"{a.layers} layers, random weights, dropout 0.1, --sp-pred, dynamic loss scale; a step of {B} x {L} rows; the evaluation of {r0['items']} chains of "
             f"{r0['questions']} questions in {r0['batches']} batches of 128; rank 0's host clocks around work that ends in a synchronise, medians of {a.steps} steps and "
             f"{a.rounds} evaluations after one warm-up each).", "",
             "## One rank against the parent commit", "",
             "The world-less path adds no call, so the expectation is no difference beyond the spread between two runs of the same code. No ratio is asserted.", "",
             "| run | whole step ms | evaluation s (decode / metrics) |", "|---|---|---|"]
    for i, r in enumerate(one):
        lines.append(f"| this commit, run {i + 1} | {r['step_ms']['whole']:.1f} | {r['eval_s']['whole']:.3f} ({r['eval_s']['decode']:.3f} / {r['eval_s']['metrics']:.3f}) |")
    for i, r in enumerate(parent):
        lines.append(f"| the parent commit, run {i + 1} | {r['step_ms']['whole']:.1f} | {r['eval_s']['whole']:.3f} ({r['eval_s']['decode']:.3f} / {r['eval_s']['metrics']:.3f}) |")
    if not parent:
        lines.append("| the parent commit | not measured in this session | |")
    lines += ["", "## The step", "",
              "| ranks | transport | train_step ms | exchange ms | mdr_rank_sum ms | publish ms | optimizer ms | whole step ms | peak GiB |", "|---|---|---|---|---|---|---|---|---|"]
    for r in [r0] + rows:
        m = r["step_ms"]
        lines.append(f"| {r['ranks']} | {r['transport']} | {m['train_step']:.1f} | {m['exchange']:.2f} | {m['rank_sum']:.3f} | {m['publish']:.2f} | {m['optimizer']:.2f} | "
                     f"{m['whole']:.1f} | {r['peak_gib']:.2f} |")
    lines += ["", "## The evaluation", "", "| ranks | transport | decode of own batches s | merge s | select + winners + metrics s | whole s |", "|---|---|---|---|---|---|"]
    for r in [r0] + rows:
        e = r["eval_s"]
        lines.append(f"| {r['ranks']} | {r['transport']} | {e['decode']:.3f} | {e['merge']:.3f} | {e['metrics']:.3f} | {e['whole']:.3f} |")
    shared = [r for r in rows if "shared" in r["transport"]]
    if shared:
        lines += ["", f"Rows marked `gloo, one shared device` are the one-card rehearsal: {devices} device was visible, all ranks queue on it and every byte exchanged crosses "
                  "the host. It is slower than one rank, as it must be; it shows what the rehearsal costs and that it runs, nothing about N devices. No run on N devices "
                  "under RCCL exists, and no speed-up is claimed."]
    lines += ["", f"Steps skipped by the loss scaler during the runs: {', '.join(str(r['skipped_total']) + ' at ' + str(r['ranks']) + ' ranks' for r in [r0] + rows)}."]
    if a.dsplit:
        lines += ["", "## d_split and d_perm per tensor (tests/test_reader_multirank_step_gpu.py::test_against_the_one_rank_step)", "", "```", open(a.dsplit).read().rstrip("\n"), "```"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
