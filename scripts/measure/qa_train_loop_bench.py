"""Measure what the reader's training loop (scripts/train_qa.py --do_train) pays for its data path, at ELECTRA-large geometry (24 x 1024,
16 heads, FFN 4096), 64 rows of 300 to 512 tokens, on one device:

    python scripts/measure/qa_train_loop_bench.py [--rows 64] [--steps 5] [--questions 32] [--out FILE.json]

A synthetic train file is written (random words of the committed tiny vocabulary, tests/golden/reader_electra_tiny/vocab.txt: no real
WordPiece vocabulary travels with the tree, so the host path tokenises with the tiny one; the ids fit the large table), the training
dataset and its arena are built from it, and three loop bodies are timed in alternation, --steps steps each after one warm-up step, a host
clock around work that ends in loss.item() and a device synchronise:
  (a) train_step + opt.step() + loss.item() on ONE resident batch: the parent commit's path, the baseline
  (b) arena.batch_shape + arena.assemble (mdr_reader_train_assemble) in front of the same body: the product's loop
  (c) the host path in front of it: dataset[i] per row, qa_train_collate, upload
and alone: the assemble kernel (device events), the host seconds of one batch of (c), the host seconds (a) spends without the loss.item()
read-back, and the arena's bytes per item. Prints one JSON object; profiles/qa_train_loop.md holds a run."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from multihop_dense_retrieval_amd import qa_train_arena, qa_train_data, reader_train  # noqa: E402

VOCAB = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny", "vocab.txt")
MAX_SEQ_LEN, MAX_Q_LEN, NEG = 512, 64, 7


def large_config():
    return types.SimpleNamespace(vocab_size=30522, hidden_size=1024, embedding_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                                 max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu", pad_token_id=0,
                                 hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)


def write_train_file(path, n_questions, rng):
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

            def chain(tag, with_answer):
                total = rng.randint(280, 520)  # the row adds [CLS] q [SEP] yes no [SEP] ... [SEP]: some rows are cut at 512
                a = rng.randint(total // 3, 2 * total // 3)
                return [passage(f"{tag} {q} a", a, answer if with_answer else None), passage(f"{tag} {q} b", total - a)]

            gold = chain("gold", True)
            item = {"_id": f"s{q}", "question": " ".join(rng.choice(words) for _ in range(rng.randint(8, 20))) + " ?", "answer": [answer], "type": "bridge",
                    "sp": [dict(p, sp_sent_ids=[0]) for p in gold], "candidate_chains": [gold] + [chain(f"neg{c}", False) for c in range(NEG)]}
            f.write(json.dumps(item) + "\n")


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--questions", type=int, default=32)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import transformers
    if not torch.cuda.is_available():
        sys.exit("this measurement needs a HIP device (there is no CPU fallback)")
    rng = random.Random(0)
    torch.manual_seed(0)
    tok = transformers.BertTokenizer(VOCAB, do_lower_case=True)
    tmp = tempfile.mkdtemp(prefix="qa_train_loop_bench_")
    train_file = os.path.join(tmp, "train.jsonl")
    write_train_file(train_file, a.questions, rng)
    ds = qa_train_data.QATrainDataset(tok, train_file, MAX_SEQ_LEN, MAX_Q_LEN)
    t0 = time.perf_counter()
    arena = qa_train_arena.QATrainArena.from_dataset(ds)
    build_s = time.perf_counter() - t0
    arena.to("cuda")
    n = arena.n
    res = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "steps": a.steps, "items": n, "arena_build_seconds": build_s,
           "arena_bytes_per_item": arena.bytes_per_item, "row_lengths": {"min": int(arena.lens.min()), "median": float(statistics.median(arena.lens.tolist())),
                                                                       "max": int(arena.lens.max())}, "tokenizer": "the committed tiny vocabulary (132 entries)"}
    args = types.SimpleNamespace(model_name="google/electra-large-discriminator", sp_pred=True, sp_weight=0.025, learning_rate=5e-5, adam_epsilon=1e-8,
                                 max_grad_norm=2.0, weight_decay=0.01, gradient_accumulation_steps=1, use_adam=False)
    model = reader_train.TrainableReader(large_config(), args).cuda().train()
    opt = reader_train.optimizer_for(model, args)
    order = list(range(n))
    rng.shuffle(order)
    batches = [order[lo:lo + a.rows] for lo in range(0, n - a.rows + 1, a.rows)]
    on_dev = torch.tensor(order, dtype=torch.int64, device="cuda")
    seed = [0]

    def body(batch, item=True):
        seed[0] += 1
        loss = reader_train.train_step(model, batch, args, opt, seed[0])
        opt.step()
        return loss.item() if item else None

    def from_arena(k):
        idx = batches[k % len(batches)]
        L, S, P = arena.batch_shape(idx)
        lo = (k % len(batches)) * a.rows
        out = arena.assemble(on_dev[lo:lo + a.rows], L, S, P, tok.pad_token_id)
        return {key: out[key] for key in qa_train_arena.NET_KEYS}

    def from_host(k):
        net = qa_train_data.qa_train_collate([ds[i] for i in batches[k % len(batches)]], pad_id=tok.pad_token_id)["net_inputs"]
        return {key: v.to(device="cuda", dtype=torch.int64) for key, v in net.items()}

    resident = from_arena(0)
    res["resident_batch"] = {"L": int(resident["input_ids"].shape[1]), "tokens": int(resident["attention_mask"].sum())}
    variants = {"a_resident": lambda k: body(resident), "b_arena": lambda k: body(from_arena(k)), "c_host": lambda k: body(from_host(k)),
                "a_resident_no_item": lambda k: body(resident, item=False)}
    times = {name: [] for name in variants}
    for k in range(a.steps + 1):
        for name, fn in variants.items():  # alternated: the three share whatever else the machine is doing
            t, _ = wall(lambda: fn(k))
            if k:  # the first step of each warms up (allocator, optimizer table, every shape's first launch)
                times[name].append(t * 1e3)
    res["step_ms"] = {name: {"median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in times.items()}
    base = res["step_ms"]["a_resident"]["median"]
    res["b_over_a"], res["c_over_a"] = res["step_ms"]["b_arena"]["median"] / base, res["step_ms"]["c_host"]["median"] / base
    # ---- the parts alone
    L, S, P = arena.batch_shape(batches[0])
    ev = []
    for _ in range(21):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        arena.assemble(on_dev[:a.rows], L, S, P, tok.pad_token_id)
        e.record()
        torch.cuda.synchronize()
        ev.append(s.elapsed_time(e))
    res["assemble_kernel_ms"] = {"median": statistics.median(ev[1:]), "min": min(ev[1:]), "bytes_written": 8 * a.rows * (4 * L + 2 * S + 2 * P + 4)}
    t_shape = []
    for k in range(20):
        t = time.perf_counter()
        arena.batch_shape(batches[k % len(batches)])
        t_shape.append((time.perf_counter() - t) * 1e3)
    res["batch_shape_host_ms"] = statistics.median(t_shape)
    res["assemble_with_sync_ms"] = statistics.median(wall(lambda: from_arena(k))[0] * 1e3 for k in range(1, 11))
    res["host_batch_ms"] = statistics.median(wall(lambda: from_host(k))[0] * 1e3 for k in range(1, 6))
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
