"""Measure the reader's training PIECE arena (multihop_dense_retrieval_amd/qa_train_pieces.py, mdr_reader_train_compose) against the item
arena it stands beside (qa_train_arena.py, mdr_reader_train_assemble), on a synthetic train file shaped like the README's
train_retrieval_b100_k100_sp.json: --questions questions, 100 candidate chains each, drawn from a per-question passage pool.

    python scripts/measure/qa_train_pieces_bench.py --part host   [--questions 200] [--out profiles/qa_train_pieces_host.json]     (no device)
    python scripts/measure/qa_train_pieces_bench.py --part device [--questions 16] [--steps 8] [--out profiles/qa_train_pieces_device.json]
    python scripts/measure/qa_train_pieces_bench.py --part report  (the two JSON files -> profiles/qa_train_pieces.md)

The words are those of the committed tiny vocabulary (tests/golden/reader_electra_tiny/vocab.txt), as in scripts/measure/qa_train_loop_bench.py:
no real WordPiece vocabulary travels with the tree. Two parameters of the real file are not known here and are therefore STATED, and more
than one value of each is reported: the pool size (it sets the ratio of distinct passages to passage instances) and the probability that a
candidate chain holds the gold passage with the answer (such a chain has ans_covered = 1 and still goes through prepare() + answer_spans).

host:   QATrainArena.from_dataset (every item's __getitem__, the parent's path) against QATrainPieces.from_dataset with workers 0 and 16,
        seconds and bytes per item, and the share of items that went through answer_spans; the arrays of workers 16 equal those of workers 0.
device: median device-event time of mdr_reader_train_compose next to mdr_reader_train_assemble on the same 64 item indices (rows cut at
        512), and the loop body of qa_train_loop_bench.py (ELECTRA-large geometry) with either arena in front, timed in alternation.
"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts", "measure"))

VOCAB = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny", "vocab.txt")
MAX_SEQ_LEN, MAX_Q_LEN, CHAINS = 512, 64, 100
CONFIGS = ((30, 0.25), (120, 0.25), (120, 0.05))  # (passages in a question's pool, P(a candidate chain holds the gold answer passage))
PROFILES = os.path.join(ROOT, "profiles")


def write_train_file(path, n_questions, pool_size, p_gold, rng):
    words = [w for w in open(VOCAB).read().split("\n") if w.isalpha() and len(w) > 1 and w not in ("yes", "no")]

    def passage(title, n_tokens, answer=None):
        sents, left = [], n_tokens
        while left > 0:
            k = min(left, rng.randint(12, 30))
            sents.append(" ".join(rng.choice(words) for _ in range(k - 1)) + " .")
            left -= k + 1  # the sentence marker
        if answer:
            sents[0] = answer + " " + sents[0]
        return {"title": title, "sents": sents}

    with open(path, "w") as f:
        for q in range(n_questions):
            answer = " ".join(rng.choice(words) for _ in range(2))
            # chains of 280 to 520 WordPieces, as qa_train_loop_bench.py's: with [CLS] q [SEP] yes no [SEP] ... [SEP] some rows are cut at 512
            gold = [passage(f"gold {q} a", rng.randint(140, 260), answer), passage(f"gold {q} b", rng.randint(140, 260))]
            pool = [passage(f"pool {q} {i}", rng.randint(140, 260)) for i in range(pool_size)]
            chains = []
            for _ in range(CHAINS):
                a, b = rng.sample(pool, 2)
                if rng.random() < p_gold:
                    a, b = (gold[0], b) if rng.random() < 0.5 else (b, gold[0])
                chains.append([a, b])
            item = {"_id": f"s{q}", "question": " ".join(rng.choice(words) for _ in range(rng.randint(8, 20))) + " ?", "answer": [answer], "type": "bridge",
                    "sp": [dict(p, sp_sent_ids=[0]) for p in gold], "candidate_chains": chains}
            f.write(json.dumps(item) + "\n")


def dataset(n_questions, pool_size, p_gold, seed=0):
    import transformers
    from multihop_dense_retrieval_amd import qa_train_data
    tok = transformers.BertTokenizer(VOCAB, do_lower_case=True)
    tmp = tempfile.mkdtemp(prefix="qa_train_pieces_bench_")
    train_file = os.path.join(tmp, "train.jsonl")
    try:
        write_train_file(train_file, n_questions, pool_size, p_gold, random.Random(seed))
        return tok, qa_train_data.QATrainDataset(tok, train_file, MAX_SEQ_LEN, MAX_Q_LEN)
    finally:
        shutil.rmtree(tmp)


def clock(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def host_part(a):
    import numpy as np
    from multihop_dense_retrieval_amd import qa_train_arena, qa_train_pieces
    res = {"questions": a.questions, "chains_per_question": CHAINS, "cpus": len(os.sched_getaffinity(0)), "configs": []}
    for pool_size, p_gold in CONFIGS:
        tok, ds = dataset(a.questions, pool_size, p_gold)
        t_item, items = clock(lambda: qa_train_arena.QATrainArena.from_dataset(ds))
        t_p0, p0 = clock(lambda: qa_train_pieces.QATrainPieces.from_dataset(ds, workers=0))
        t_p16, p16 = clock(lambda: qa_train_pieces.QATrainPieces.from_dataset(ds, workers=16))
        same = all(getattr(p0, n).tobytes() == getattr(p16, n).tobytes() for n, _ in qa_train_pieces._ARRAYS)
        idx = list(range(0, items.n, max(1, items.n // 257)))
        want, got = items.assemble_host(idx), p0.compose_host(idx)
        res["configs"].append({"pool": pool_size, "p_gold": p_gold, "items": items.n, "distinct_passages": p0.n_passages,
                               "distinct_over_instances": p0.n_passages / (2 * items.n), "share_through_answer_spans": p0.searched / items.n,
                               "share_cut_at_512": float((items.lens >= MAX_SEQ_LEN).mean()),
                               "item_arena": {"seconds": t_item, "ms_per_item": 1e3 * t_item / items.n, "bytes_per_item": items.bytes_per_item},
                               "pieces_workers_0": {"seconds": t_p0, "ms_per_item": 1e3 * t_p0 / items.n, "bytes_per_item": p0.bytes_per_item},
                               "pieces_workers_16": {"seconds": t_p16, "ms_per_item": 1e3 * t_p16 / items.n},
                               "workers_16_arrays_equal_workers_0": same,
                               "rows_equal_the_item_arena": all(np.array_equal(want[k], got[k]) for k in want),
                               "faster_with_workers_0": t_p0 < t_item, "factor_workers_0": t_item / t_p0, "factor_workers_16": t_item / t_p16,
                               "bytes_factor": items.bytes_per_item / p0.bytes_per_item})
        print(json.dumps(res["configs"][-1]), flush=True)
    return res


def device_part(a):
    import torch
    import qa_train_loop_bench as loop
    from multihop_dense_retrieval_amd import qa_train_arena, qa_train_pieces, reader_train
    if not torch.cuda.is_available():
        sys.exit("this part needs a HIP device (there is no CPU fallback)")
    pool_size, p_gold = CONFIGS[0]
    tok, ds = dataset(a.questions, pool_size, p_gold)  # built before the device is opened
    items, pieces = qa_train_arena.QATrainArena.from_dataset(ds), qa_train_pieces.QATrainPieces.from_dataset(ds)
    torch.manual_seed(0)
    items.to("cuda")
    pieces.to("cuda")
    n, rows = items.n, a.rows
    rng = random.Random(0)
    order = list(range(n))
    rng.shuffle(order)
    batches = [order[lo:lo + rows] for lo in range(0, n - rows + 1, rows)]
    on_dev = torch.tensor(order, dtype=torch.int64, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "rows": rows, "steps": a.steps, "items": n, "pool": pool_size, "p_gold": p_gold}
    # ---- the two kernels alone, on the same indices
    L, S, P = items.batch_shape(batches[0])
    assert (L, S, P) == pieces.batch_shape(batches[0])
    one, two = items.assemble(on_dev[:rows], L, S, P, tok.pad_token_id), pieces.assemble(on_dev[:rows], L, S, P, tok.pad_token_id)
    res["kernels_give_equal_tensors"] = all(torch.equal(one[k], two[k]) for k in one)
    res["kernel_shape"] = {"rows": rows, "L": L, "n_sent": S, "n_span": P, "bytes_written": 8 * rows * (4 * L + 2 * S + 2 * P + 4)}
    for name, arena in (("mdr_reader_train_assemble", items), ("mdr_reader_train_compose", pieces)):
        ev = []
        for _ in range(21):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            arena.assemble(on_dev[:rows], L, S, P, tok.pad_token_id)
            e.record()
            torch.cuda.synchronize()
            ev.append(s.elapsed_time(e))
        res[name + "_ms"] = {"median": statistics.median(ev[1:]), "min": min(ev[1:]), "max": max(ev[1:])}
    res["compose_over_assemble"] = res["mdr_reader_train_compose_ms"]["median"] / res["mdr_reader_train_assemble_ms"]["median"]
    # ---- the loop body with either arena in front
    args = types.SimpleNamespace(model_name="google/electra-large-discriminator", sp_pred=True, sp_weight=0.025, learning_rate=5e-5, adam_epsilon=1e-8,
                                 max_grad_norm=2.0, weight_decay=0.01, gradient_accumulation_steps=1, use_adam=False)
    model = reader_train.TrainableReader(loop.large_config(), args).cuda().train()
    opt = reader_train.optimizer_for(model, args)
    seed = [0]

    def body(batch):
        seed[0] += 1
        loss = reader_train.train_step(model, batch, args, opt, seed[0])
        opt.step()
        return loss.item()

    def feed(arena, k):
        idx = batches[k % len(batches)]
        lo = (k % len(batches)) * rows
        out = arena.assemble(on_dev[lo:lo + rows], *arena.batch_shape(idx), tok.pad_token_id)
        return {key: out[key] for key in qa_train_arena.NET_KEYS}

    variants = {"item_arena": lambda k: body(feed(items, k)), "piece_arena": lambda k: body(feed(pieces, k))}
    times = {name: [] for name in variants}
    for k in range(a.steps + 1):
        for name, fn in variants.items():  # alternated: both walk the same batches and share whatever else the machine is doing
            t, _ = loop.wall(lambda: fn(k))
            if k:  # the first step of each warms up
                times[name].append(t * 1e3)
    res["step_ms"] = {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for name, v in times.items()}
    it, pc = res["step_ms"]["item_arena"], res["step_ms"]["piece_arena"]
    res["piece_median_inside_item_spread"] = it["min"] <= pc["median"] <= it["max"]
    return res


def report():
    h = json.load(open(os.path.join(PROFILES, "qa_train_pieces_host.json")))
    d = json.load(open(os.path.join(PROFILES, "qa_train_pieces_device.json")))
    lines = ["# The reader's training feed from a piece arena", "",
             "`scripts/measure/qa_train_pieces_bench.py` (this file is its `--part report`; the numbers are in `profiles/qa_train_pieces_host.json` and",
             "`profiles/qa_train_pieces_device.json`). The synthetic train file is `scripts/measure/qa_train_loop_bench.py`'s (random words of the committed",
             f"tiny vocabulary, chains of 280 to 520 WordPieces, `max_seq_len` 512), shaped like the README's training file: {h['questions']} questions, 100",
             "candidate chains each, drawn from a per-question passage pool. Two properties of the real file are not known here, so they are parameters",
             "and not claims: the pool size, which sets the ratio of distinct passages to passage instances, and the probability that a candidate",
             "chain holds the gold passage with the answer (such a chain has `ans_covered = 1` and still goes through `prepare()` + `answer_spans`).", "",
             f"## Building the arena on the host ({h['cpus']} CPUs, no device)", "",
             "| pool, P(gold passage) | items | distinct / instances | through `answer_spans` | cut at 512 | item arena (the parent's path) | pieces, workers 0 | pieces, workers 16 | bytes per item: item arena, pieces |",
             "|---|---|---|---|---|---|---|---|---|"]
    for c in h["configs"]:
        lines.append(f"| {c['pool']}, {c['p_gold']} | {c['items']} | {c['distinct_over_instances']:.3f} | {100 * c['share_through_answer_spans']:.1f} % | "
                     f"{100 * c['share_cut_at_512']:.1f} % | {c['item_arena']['seconds']:.1f} s ({c['item_arena']['ms_per_item']:.2f} ms per item) | "
                     f"{c['pieces_workers_0']['seconds']:.1f} s ({c['pieces_workers_0']['ms_per_item']:.2f} ms per item, {c['factor_workers_0']:.1f} x) | "
                     f"{c['pieces_workers_16']['seconds']:.1f} s ({c['factor_workers_16']:.1f} x) | {c['item_arena']['bytes_per_item']:.0f}, "
                     f"{c['pieces_workers_0']['bytes_per_item']:.0f} ({c['bytes_factor']:.1f} x) |")
    ok = all(c["faster_with_workers_0"] and c["workers_16_arrays_equal_workers_0"] and c["rows_equal_the_item_arena"] for c in h["configs"])
    item_ms, p0_ms, p16_ms = ([c[k]["ms_per_item"] for c in h["configs"]] for k in ("item_arena", "pieces_workers_0", "pieces_workers_16"))  # (x 9e6 / 3.6e6 = hours; / 6e4 = minutes)
    p_bytes = [c["pieces_workers_0"]["bytes_per_item"] for c in h["configs"]]
    lines += ["", f"What must hold, holds: {ok} -- the build with `workers = 0` is faster than the parent's on every row, the arrays of `workers = 16` are bit-equal to",
              "those of `workers = 0`, and 257 rows spread over each file compose to the item arena's rows (`compose_host` against `assemble_host`).", "",
              "Where the time goes: a question is tokenised once and a passage once, so that part shrinks with the distinct / instances ratio; the items",
              "with `ans_covered = 1` and a span answer still run `prepare()`'s character loop over the whole chain and `answer_spans`, under a memo of",
              "`tokenizer.tokenize` per distinct string, and they are what is left: the build time follows the share in the fourth column. The tiny",
              "vocabulary flatters both paths alike (most words are one piece).", "",
              f"Extrapolated, NOT measured: at 9 M items (90 k questions x 100 chains) the item arena's rates are {min(item_ms) * 2.5:.1f} to {max(item_ms) * 2.5:.1f} hours of one process",
              f"and {max(c['item_arena']['bytes_per_item'] for c in h['configs']) * 9e6 / 1e9:.0f} GB; the piece arena's rates with 16 workers on these {h['cpus']} CPUs are "
              f"{min(p16_ms) * 150:.0f} to {max(p16_ms) * 150:.0f} minutes, with `workers = 0` {min(p0_ms) * 150:.0f} to {max(p0_ms) * 150:.0f} minutes, and "
              f"{min(p_bytes) * 9e6 / 1e9:.1f} to {max(p_bytes) * 9e6 / 1e9:.1f} GB,",
              "over these rows' parameters. The real file's two ratios decide where in (or outside) those ranges a run lands; reading the 9 M records into",
              "`QATrainDataset` comes before either arena and is not part of these figures.", "",
              f"## On the device (one MI355X; torch names it `{d['device']}`)", "",
              f"{d['items']} items (pool {d['pool']}, P(gold passage) {d['p_gold']}), {d['rows']} item indices, out_len {d['kernel_shape']['L']}, n_sent {d['kernel_shape']['n_sent']}, "
              f"n_span {d['kernel_shape']['n_span']} ({d['kernel_shape']['bytes_written'] / 1e6:.2f} MB written); the two kernels gave equal tensors: {d['kernels_give_equal_tensors']}.", "",
              "| kernel, device events, median of 20 (min .. max) | ms |", "|---|---|"]
    for name in ("mdr_reader_train_assemble", "mdr_reader_train_compose"):
        k = d[name + "_ms"]
        lines.append(f"| `{name}` | {k['median']:.4f} ({k['min']:.4f} .. {k['max']:.4f}) |")
    lines += ["", f"compose / assemble = {d['compose_over_assemble']:.2f}. Both are launch-bound integer copies; compose reads five index entries per row before its first token "
              "(item, then question and passage offsets: two dependent loads where assemble has one) and compacts the spans with a ballot and one barrier pair.", "",
              f"The loop body of `scripts/measure/qa_train_loop_bench.py` (ELECTRA-large geometry, {d['rows']} rows, `train_step` + `opt.step()` + `loss.item()`), either arena in front,",
              f"{d['steps']} steps each after one warm-up step, in alternation over the same batches:", "",
              "| feed | ms per step: median (min .. max) |", "|---|---|"]
    for name in ("item_arena", "piece_arena"):
        s = d["step_ms"][name]
        lines.append(f"| {name.replace('_', ' ')} | {s['median']:.2f} ({s['min']:.2f} .. {s['max']:.2f}) |")
    lines += ["", f"The piece arena's median lies inside the item arena's min .. max: {d['piece_median_inside_item_spread']}.", ""]
    open(os.path.join(PROFILES, "qa_train_pieces.md"), "w").write("\n".join(lines))
    print(os.path.join(PROFILES, "qa_train_pieces.md"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("host", "device", "report"), required=True)
    ap.add_argument("--questions", type=int, default=0)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.part == "report":
        return report()
    a.questions = a.questions or (200 if a.part == "host" else 16)
    res = host_part(a) if a.part == "host" else device_part(a)
    text = json.dumps(res, indent=1)
    print(text)
    out = a.out or os.path.join(PROFILES, f"qa_train_pieces_{a.part}.json")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    open(out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
