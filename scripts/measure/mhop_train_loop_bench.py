"""Measure what retriever training (scripts/train_mhop.py and scripts/train_momentum.py --do_train) pays for its data path, at roberta-base
geometry, 150 samples a step, the cuts 70 / 350 / 300, on one device:

    python scripts/measure/mhop_train_loop_bench.py [--batch 150] [--rounds 5] [--train 600] [--dev 3000] [--out FILE.json]

A synthetic train file and a synthetic dev file are written (random words through the committed tiny BPE, tests/golden/tiny_bpe: no real
RoBERTa vocabulary travels with the tree, so the host path tokenises with the tiny one; the ids fit the large table). Passages are encoded to
150 .. 300 tokens, questions to 35 .. 70, question + start passage pairs are cut at 350: the length distribution of
scripts/measure/train_step_bench.py. Every third sample is a comparison question; a train sample has five tfidf negatives.

For the momentum step (multihop_dense_retrieval_amd/momentum.py, --k 76800) and then for the plain step (multihop_dense_retrieval_amd/train.py),
three loop bodies are timed in alternation, --rounds rounds after one warm-up round, each body = batch + train_step + opt.step() +
loss.item(), a host clock around it and a device synchronise:
  (a) resident   the epoch's batches assembled beforehand and kept on the device
  (b) arena      MhopArena.choose + the row table's copy + mdr_mhop_assemble in front of the step: the product's loop
  (c) host       MhopTrainDataset.__getitem__ per sample + mhop_collate + upload in front of it: the reference's loop
all three walk the same index batches. Alone: the kernel (device events), choose (host clock), choose + copy + kernel with a synchronise,
the host path of one batch, the arena's bytes per sample and build seconds per sample, and ONE dev evaluation of --dev samples
(--predict_batch_size 3000, the six inference forwards and the ranks) by both feeds, the second of two passes each.
Prints one JSON object; profiles/mhop_train_loop.md holds a run."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time
import types
from functools import partial

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from multihop_dense_retrieval_amd import criterions, data, mhop_arena, mhop_data, momentum, retriever, train  # noqa: E402
from multihop_dense_retrieval_amd.retriever import move_to_cuda  # noqa: E402

BPE = os.path.join(ROOT, "tests", "golden", "tiny_bpe")
MAX_Q_LEN, MAX_Q_SP_LEN, MAX_C_LEN = 70, 350, 300
WORDS = ("the quick brown fox jumps over lazy dog river bank retrieval encoder index beam passage question answer Paris London film band "
         "album studio producer capital France Seine stadium people author born city population 1950 2012 80,000 3.14").split()
TOKENS_PER_WORD = 1.15  # of WORDS under the tiny BPE


def tiny_tokenizer(tmp):
    import transformers
    vocab = json.load(open(os.path.join(BPE, "vocab.json")))
    merges = [tuple(ln.split()) for ln in open(os.path.join(BPE, "merges.txt")).read().split("\n") if ln and not ln.startswith("#")]
    d = os.path.join(tmp, "tok")
    transformers.RobertaTokenizer(vocab=vocab, merges=merges).save_pretrained(d)
    return data.load_tokenizer(d)


def write_file(path, n, rng, n_neg, key):
    text = lambda lo, hi: " ".join(rng.choice(WORDS) for _ in range(int(rng.randint(lo, hi) / TOKENS_PER_WORD)))  # noqa: E731
    with open(path, "w") as f:
        for i in range(n):
            para = lambda tag: {"title": f"{tag} {i} " + text(2, 4), "text": text(140, 290)}  # noqa: E731
            s = {"question": text(33, 66) + "?", "type": "comparison" if i % 3 == 0 else "bridge", "pos_paras": [para("Start"), para("Bridge")],
                 "neg_paras": [para("Neg a"), para("Neg b")]}
            if key == "tfidf_neg":
                s["tfidf_neg"] = [para(f"Tfidf {k}") for k in range(n_neg)]
            if s["type"] != "comparison":
                s["bridge"] = s["pos_paras"][1]["title"]
            f.write(json.dumps(s) + ("\n" if i + 1 < n else ""))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "each": [round(x, 3) for x in v]}


def time_steps(steps, model, args, opt, arena, ds, batches, rounds):
    """The three loop bodies over the same index batches, alternated; ms per step."""
    collate = partial(mhop_data.mhop_collate, pad_id=0)
    feed = arena.feed(len(batches[0]), shuffle=False)
    seed = [0]

    def body(batch):
        seed[0] += 1
        loss = steps.train_step(model, move_to_cuda(batch), args, opt, seed[0])
        opt.step()
        return loss.item()

    def from_arena(k):
        table, widths = arena.choose(batches[k % len(batches)])
        return arena.assemble(feed.upload(table), widths)

    def from_host(k):
        return collate([ds[i] for i in batches[k % len(batches)]])

    resident = [from_arena(k) for k in range(len(batches))]
    variants = {"a_resident": lambda k: body(resident[k % len(batches)]), "b_arena": lambda k: body(from_arena(k)), "c_host": lambda k: body(from_host(k))}
    times = {name: [] for name in variants}
    for k in range(rounds + 1):
        for name, fn in variants.items():  # alternated: the three share whatever else the machine is doing
            t, _ = wall(lambda: fn(k))
            if k:  # the first round warms up (allocator, optimizer table, every shape's first launch)
                times[name].append(t)
    out = {name: spread(v) for name, v in times.items()}
    out["tokens_per_batch"] = [int(sum(int(b[f"{s}_mask"].sum()) for s in mhop_arena.SLOTS)) for b in resident]
    out["skipped_total"] = opt.read_state()["skipped_total"]
    return out, from_arena, from_host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--train", type=int, default=600)
    ap.add_argument("--dev", type=int, default=3000)
    ap.add_argument("--k", type=int, default=76800)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this measurement needs a HIP device (there is no CPU fallback)")
    rng = random.Random(0)
    random.seed(0)
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp(prefix="mhop_train_loop_bench_")
    tok = tiny_tokenizer(tmp)
    train_file, dev_file = os.path.join(tmp, "train.jsonl"), os.path.join(tmp, "dev.jsonl")
    write_file(train_file, a.train, rng, 5, "tfidf_neg")
    write_file(dev_file, a.dev, rng, 2, "neg_paras")
    cuts = (MAX_Q_LEN, MAX_Q_SP_LEN, MAX_C_LEN)
    ds = mhop_data.MhopTrainDataset(tok, train_file, *cuts)
    arena = mhop_arena.MhopArena.from_dataset(ds).to("cuda")
    dev_ds = mhop_data.MhopDataset(tok, dev_file, *cuts)
    dev_arena = mhop_arena.MhopArena.from_dataset(dev_ds).to("cuda")
    part = lambda lo, hi: arena.lens[lo:hi]  # noqa: E731
    n_pass = arena.n_rows - arena.n - int((arena.qsp_rows >= 0).sum())
    lens = {"q": part(0, arena.n), "passage": part(arena.n, arena.n + n_pass), "q_sp": part(arena.n + n_pass, arena.n_rows)}
    res = {"device": torch.cuda.get_device_name(0), "batch": a.batch, "rounds": a.rounds, "tokenizer": "the committed tiny BPE (587 entries)",
           "train": {"samples": arena.n, "rows": arena.n_rows, "bytes_per_sample": arena.bytes_per_sample, "build_seconds": arena.build_seconds,
                     "build_ms_per_sample": arena.build_seconds / arena.n * 1e3},
           "dev": {"samples": dev_arena.n, "rows": dev_arena.n_rows, "bytes_per_sample": dev_arena.bytes_per_sample, "build_seconds": dev_arena.build_seconds,
                   "build_ms_per_sample": dev_arena.build_seconds / dev_arena.n * 1e3},
           "row_lengths": {k: {"min": int(v.min()), "median": float(statistics.median(v.tolist())), "max": int(v.max())} for k, v in lens.items()}}
    order = list(range(arena.n))
    rng.shuffle(order)
    batches = [order[lo:lo + a.batch] for lo in range(0, arena.n - a.batch + 1, a.batch)]
    cfg = retriever.RobertaConfig()
    cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = 0.1, 0.1
    base = dict(adam_epsilon=1e-8, max_grad_norm=2.0, weight_decay=0.0, gradient_accumulation_steps=1, fp16=True)

    # ---- the momentum step
    args = types.SimpleNamespace(learning_rate=1e-5, momentum=True, k=a.k, m=0.999, init_retriever="", **base)
    model = momentum.MomentumRetriever(cfg, args).cuda().train()
    opt = momentum.optimizer_for(model, args)
    res["momentum_step_ms"], _, _ = time_steps(momentum, model, args, opt, arena, ds, batches, a.rounds)
    del model, opt
    torch.cuda.empty_cache()

    # ---- the plain step
    args = types.SimpleNamespace(learning_rate=2e-5, momentum=False, **base)
    model = train.TrainableRetriever(cfg, args).cuda().train()
    opt = train.optimizer_for(model, args)
    res["plain_step_ms"], from_arena, from_host = time_steps(train, model, args, opt, arena, ds, batches, a.rounds)

    # ---- the parts alone
    table, widths = arena.choose(batches[0])
    on_dev = torch.from_numpy(table).cuda()
    ev = []
    for _ in range(21):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        arena.assemble(on_dev, widths)
        e.record()
        torch.cuda.synchronize()
        ev.append(s.elapsed_time(e))
    res["assemble_kernel_ms"] = {"median": statistics.median(ev[1:]), "min": min(ev[1:]), "widths": list(widths), "bytes_written": 16 * a.batch * sum(widths),
                                 "table_bytes": int(table.nbytes)}
    t_choose = []
    for k in range(20):
        t = time.perf_counter()
        arena.choose(batches[k % len(batches)])
        t_choose.append((time.perf_counter() - t) * 1e3)
    res["choose_host_ms"] = spread(t_choose)
    res["arena_batch_with_sync_ms"] = spread([wall(lambda: from_arena(k))[0] for k in range(1, 11)])
    res["host_batch_ms"] = spread([wall(lambda: move_to_cuda(from_host(k)))[0] for k in range(1, 6)])

    # ---- one dev evaluation by both feeds
    infer = model.inference()
    del opt
    torch.cuda.empty_cache()
    collate = partial(mhop_data.mhop_collate, pad_id=0)
    feeds = {"arena": dev_arena.feed(3000, shuffle=False),
             "host": torch.utils.data.DataLoader(dev_ds, batch_size=3000, collate_fn=collate, num_workers=0)}

    def evaluate(feed):
        rrs = []
        for batch in feed:
            with torch.no_grad():
                rrs += criterions.mhop_eval(infer(move_to_cuda(batch)), args)["rrs_1"]
        return len(rrs)

    dev_ms = {name: [] for name in feeds}
    for _ in range(2):
        for name, feed in feeds.items():
            t, n = wall(lambda: evaluate(feed))
            assert n == dev_arena.n
            dev_ms[name].append(t)
    res["dev_evaluation_ms"] = {name: {"first": v[0], "second": v[1]} for name, v in dev_ms.items()}
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
