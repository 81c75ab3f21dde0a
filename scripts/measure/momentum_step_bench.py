"""Time one momentum training step (multihop_dense_retrieval_amd/momentum.py) and write profiles/momentum_train_step.md:

    python scripts/measure/momentum_step_bench.py [--out profiles/momentum_train_step.md] [--steps 5] [--batch 150] [--k 76800]

roberta-base geometry with random weights, dropout 0.1 at every site, --fp16 scores, the dynamic loss scale, --max_c_len 300 / --max_q_len 70
/ --max_q_sp_len 350 (the inputs of scripts/measure/train_step_bench.py: c1, c2, neg_1, neg_2 padded to 300, q to 70, q_sp1 to 350, lengths
uniform in [L / 2, L]), 150 samples, a queue of 76800 rows. One child process under a time limit. A step is split into the two question
forwards, the four key forwards, the loss (queue.clone() included, which is timed alone as well), the backward and the optimizer step, each
by a host clock around work that ends in a device synchronise; the unsplit step is timed too; medians of --steps steps after 2 warm-up
steps; torch's peak allocated bytes of a step.

The four key forwards are also timed through both paths in one process, alternating: mdr_encoder_forward_dropout on the inference handle
(momentum.encode_dropout) against TrainableRetriever.encode under torch.no_grad() on a second set of the same weights, after a warm-up of
each, with the four outputs compared bit for bit at this size. `--relative` (optional) gives the first-step loss deviation from the
reference that tests/test_momentum_step_gpu.py measured, to be recorded beside the timings.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LENS = {"q": 70, "q_sp": 350, "c1": 300, "c2": 300, "neg1": 300, "neg2": 300}
CHILD_LIMIT_S = 540
WARMUP = 2
AB_ROUNDS = 7


def median(v):
    return sorted(v)[len(v) // 2]


def child(B, K, steps):
    import types
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import criterions, momentum, retriever, train
    torch.manual_seed(0)
    cfg = retriever.RobertaConfig()
    cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = 0.1, 0.1
    args = types.SimpleNamespace(learning_rate=1e-5, adam_epsilon=1e-8, max_grad_norm=2.0, weight_decay=0.0, gradient_accumulation_steps=1, fp16=True,
                                 momentum=True, k=K, m=0.999, init_retriever="")
    model = momentum.MomentumRetriever(cfg, args).cuda().train()
    opt = momentum.optimizer_for(model, args)
    rng = np.random.default_rng(B)
    batch, tokens = {}, {}
    for key, L in LENS.items():
        lens = rng.integers(L // 2, L + 1, size=B)
        ids = rng.integers(3, cfg.vocab_size, size=(B, L))
        mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
        ids = np.where(mask == 1, ids, 0)
        ids[:, 0] = 0
        batch[f"{key}_input_ids"], batch[f"{key}_mask"] = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
        tokens[key] = int(lens.sum())
    res = {"B": B, "K": K, "tokens": tokens}
    sync = torch.cuda.synchronize
    T_hid, T_att = model.thresholds()
    pair = lambda key: (batch[f"{key}_input_ids"], batch[f"{key}_mask"])  # noqa: E731
    parts = {k: [] for k in ("q_forwards", "key_forwards", "loss", "queue_clone", "backward", "optimizer", "whole")}
    mem = {}
    for i in range(WARMUP + steps):
        seed = 100 + i
        sync()
        torch.cuda.reset_peak_memory_stats()
        mem["before"] = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        out = {name: model.encoder_q.encode(*pair(key), opt.half, (seed, train.ENCODE_INDEX[name])) for name, key in momentum.Q_INPUTS}
        sync()
        t1 = time.perf_counter()
        with torch.no_grad():
            out.update({name: momentum.encode_dropout(model.encoder_k, *pair(key), T_hid, T_att, seed, train.ENCODE_INDEX[name]) for name, key in momentum.K_INPUTS})
        sync()
        t2 = time.perf_counter()
        loss = criterions.mhop_loss_outputs(out, args, queue=model.queue.clone())
        model.dequeue_and_enqueue(torch.cat([out["c1"], out["c2"]]).detach())
        sync()
        t3 = time.perf_counter()
        opt.scale_loss(loss).backward()
        sync()
        t4 = time.perf_counter()
        del out, loss
        opt.step()
        sync()
        t5 = time.perf_counter()
        mem["peak"] = torch.cuda.max_memory_allocated()
        model.queue.clone()
        sync()
        t6 = time.perf_counter()
        momentum.train_step(model, batch, args, opt, 200 + i)  # the same step unsplit: one synchronise at the end
        opt.step()
        sync()
        t7 = time.perf_counter()
        if i >= WARMUP:
            for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t6 - t5, t4 - t3, t5 - t4, t7 - t6)):
                parts[k].append(v * 1e3)
    res["ms"] = {k: median(v) for k, v in parts.items()}
    res["mem"] = mem
    res["skipped_total"] = opt.read_state()["skipped_total"]
    res["queue_bytes"] = model.queue.numel() * 4
    # the four key forwards through both paths, alternating, on the same weights
    chain = train.TrainableRetriever(cfg, args)
    chain.load_state_dict({k: v.detach() for k, v in model.encoder_q.state_dict().items()})
    chain = chain.cuda().train()
    key_encoder = chain.inference()  # (encoder_q has been stepped since encoder_k was copied; both paths here read the same masters)

    def fused(seed):
        return [momentum.encode_dropout(key_encoder, *pair(key), T_hid, T_att, seed, train.ENCODE_INDEX[name]) for name, key in momentum.K_INPUTS]

    def chained(seed):
        with torch.no_grad():
            return [chain.encode(*pair(key), None, (seed, train.ENCODE_INDEX[name])) for name, key in momentum.K_INPUTS]

    same = all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(fused(7), chained(7)))  # (also the warm-up of both)
    res["key_forwards_same_bits"] = same
    ab = {"fused": [], "chained": []}
    for i in range(AB_ROUNDS):
        for name, fn in (("fused", fused), ("chained", chained)):
            sync()
            t0 = time.perf_counter()
            fn(300 + i)
            sync()
            ab[name].append((time.perf_counter() - t0) * 1e3)
    res["ab_ms"] = {k: {"median": median(v), "min": min(v), "max": max(v)} for k, v in ab.items()}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "momentum_train_step.md"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=150)
    ap.add_argument("--k", type=int, default=76800)
    ap.add_argument("--relative", type=str, default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.batch, a.k, a.steps)
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--batch", str(a.batch),
           "--k", str(a.k)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        print(f"exit {p.returncode}\n{p.stderr[-3000:]}", flush=True)
        sys.exit(1)
    r = json.loads(p.stdout.strip().split("\n")[-1])
    print(r, flush=True)
    m, mem, ab = r["ms"], r["mem"], r["ab_ms"]
    gib = lambda b: f"{b / 2 ** 30:.2f}"  # noqa: E731
    total = m["q_forwards"] + m["key_forwards"] + m["loss"] + m["backward"] + m["optimizer"]
    tk = r["tokens"]
    lines = ["# One momentum training step of the retriever", "",
             f"Command: `python scripts/measure/momentum_step_bench.py --steps {a.steps} --batch {r['B']} --k {r['K']}` (roberta-base geometry, random weights, "
             "dropout 0.1, fp16 scores, dynamic loss scale; c1 / c2 / neg_1 / neg_2 padded to 300, q to 70, q_sp1 to 350, lengths uniform in [L / 2, L]; one "
             f"MI355X; host clock around work that ends in a synchronise, medians of {a.steps} steps after {WARMUP} warm-up steps; `whole` is the same step "
             "without the inner synchronises).", "",
             f"Tokens: q {tk['q']}, q_sp1 {tk['q_sp']}, c1 {tk['c1']}, c2 {tk['c2']}, neg_1 {tk['neg1']}, neg_2 {tk['neg2']}.", "",
             "| samples | queue rows | two q forwards ms | four key forwards ms | loss ms | backward ms | optimizer ms | sum ms | whole step ms | samples / s |",
             "|---|---|---|---|---|---|---|---|---|---|",
             f"| {r['B']} | {r['K']} | {m['q_forwards']:.1f} | {m['key_forwards']:.1f} | {m['loss']:.2f} | {m['backward']:.1f} | {m['optimizer']:.2f} | {total:.1f} | "
             f"{m['whole']:.1f} | {r['B'] / m['whole'] * 1e3:.1f} |", "",
             f"The loss column holds the per-step `queue.clone()` of {r['queue_bytes'] / 1e6:.0f} MB and the enqueue; the clone alone takes {m['queue_clone']:.2f} ms.",
             "", f"Allocated memory (GiB, torch's allocator): {gib(mem['before'])} before the step (encoder_q's masters, Adam's moments, fp16 copies, gradients, "
             f"the queue; encoder_k's fp16 copy lives in the library), {gib(mem['peak'])} at the peak of the step. The plain step of "
             "`profiles/train_step.md` at 150 samples: 300 ms and 65.4 GiB.", "",
             "## The four key forwards: the training-mode forward of the inference encoder against the training chain under no_grad", "",
             f"One process, the same weights, alternating, {AB_ROUNDS} rounds after a warm-up of each; host clock around the four forwards and a synchronise.", "",
             "| path | median ms | min ms | max ms |", "|---|---|---|---|",
             f"| `momentum.encode_dropout` (mdr_encoder_forward_dropout) | {ab['fused']['median']:.1f} | {ab['fused']['min']:.1f} | {ab['fused']['max']:.1f} |",
             f"| `TrainableRetriever.encode` under `torch.no_grad()` | {ab['chained']['median']:.1f} | {ab['chained']['min']:.1f} | {ab['chained']['max']:.1f} |", "",
             f"The four outputs of the two paths at this size have the same bits: {r['key_forwards_same_bits']}.", "",
             f"Steps skipped by the loss scaler during the run: {r['skipped_total']}."]
    if a.relative:
        lines += ["", "## First-step loss against the reference", "",
                  f"`tests/test_momentum_step_gpu.py::test_first_step_loss_against_the_references` (the golden first train batch, the golden initial queue, the toy "
                  f"checkpoint, dropout 0, fp32 scores): {a.relative}"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
