"""Time one training step of the retriever (multihop_dense_retrieval_amd/train.py) and write profiles/train_step.md:

    python scripts/measure/train_step_bench.py [--out profiles/train_step.md] [--steps 5]

roberta-base geometry with random weights, dropout 0.1 at every site, --fp16 scores, the dynamic loss scale; 8, 38 and 150 samples per
batch with --max_c_len 300 / --max_q_len 70 / --max_q_sp_len 350 (c1, c2, neg_1, neg_2 padded to 300, q to 70, q_sp1 to 350), sequence
lengths uniform in [L / 2, L]. One child process per batch size, under a time limit; the first failure stops the run. A step is split into
the six forwards, the loss, the backward and the optimizer step, each by a host clock around work that ends in a device synchronise (so the
parts carry a synchronise each and their sum is a little above an unsplit step, which is timed too); medians of --steps steps after 2
warm-up steps. Memory: torch's allocated bytes before the step, after the six forwards (what the graph keeps alive) and at the peak. If a
batch size does not fit, the child says so and the next smaller size of FALLBACK is tried. Also: the head's backward alone
(mdr_head_backward at [B, 768] x [768, 768], device events, median of 50), and what the per-encode torch.cat of the query / key / value
leaves costs -- the concatenations of one step's 6 x 12 Linears (weights, biases and fp16 copies) forward, and forward + backward (the split
and the accumulation into the three leaves' .grad) -- as a share of the unsplit step.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BATCHES = (8, 38, 150)
FALLBACK = (128, 112, 96, 80, 64, 48)  # tried in turn when 150 does not fit
LENS = {"q": 70, "q_sp": 350, "c1": 300, "c2": 300, "neg1": 300, "neg2": 300}
CHILD_LIMIT_S = 420
WARMUP = 2


def median(v):
    return sorted(v)[len(v) // 2]


def child(B, steps):
    import types
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import criterions, head, retriever, train
    torch.manual_seed(0)
    cfg = retriever.RobertaConfig()
    cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = 0.1, 0.1
    args = types.SimpleNamespace(learning_rate=2e-5, adam_epsilon=1e-8, max_grad_norm=2.0, weight_decay=0.0, gradient_accumulation_steps=1, fp16=True,
                                 momentum=False)
    res = {"B": B}
    try:
        model = train.TrainableRetriever(cfg, args).cuda().train()
        opt = train.optimizer_for(model, args)
        rng = np.random.default_rng(B)
        batch, tokens = {}, 0
        for key, L in LENS.items():
            lens = rng.integers(L // 2, L + 1, size=B)
            ids = rng.integers(3, cfg.vocab_size, size=(B, L))
            mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
            ids = np.where(mask == 1, ids, 0)
            ids[:, 0] = 0
            batch[f"{key}_input_ids"], batch[f"{key}_mask"] = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
            tokens += int(lens.sum())
        res["tokens"] = tokens
        sync = torch.cuda.synchronize
        parts = {k: [] for k in ("forward6", "loss", "backward", "optimizer", "whole")}
        mem = {}
        for i in range(WARMUP + steps):
            sync()
            torch.cuda.reset_peak_memory_stats()
            mem["before"] = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            out = model(batch, seed=100 + i, half=opt.half)
            sync()
            t1 = time.perf_counter()
            mem["after_forward"] = torch.cuda.memory_allocated()
            loss = criterions.mhop_loss_outputs(out, args)
            sync()
            t2 = time.perf_counter()
            opt.scale_loss(loss).backward()
            sync()
            t3 = time.perf_counter()
            del out, loss
            opt.step()
            sync()
            t4 = time.perf_counter()
            mem["peak"] = torch.cuda.max_memory_allocated()
            # the same step unsplit: one synchronise at the end
            train.train_step(model, batch, args, opt, 200 + i)
            opt.step()
            sync()
            t5 = time.perf_counter()
            if i >= WARMUP:
                for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
                    parts[k].append(v * 1e3)
        res["ms"] = {k: median(v) for k, v in parts.items()}
        res["mem"] = mem
        res["skipped_total"] = opt.read_state()["skipped_total"]
        # the head's backward alone
        H = cfg.hidden_size
        x = torch.randn(B, H, device="cuda").half()
        w = (0.02 * torch.randn(H, H, device="cuda")).half()
        dy, dw, db = torch.randn(B, H, device="cuda"), torch.empty(H, H, device="cuda"), torch.empty(H, device="cuda")
        ts = []
        for i in range(53):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            head.head_backward(x, w, dy, True, dw, db)
            b.record()
            sync()
            if i >= 3:
                ts.append(a.elapsed_time(b))
        res["head_backward_ms"] = median(ts)
        # the per-encode concatenation of the query / key / value leaves: 6 encodes x layers
        P = model.leaves()
        trip = [[P[f"encoder.encoder.layer.{i}.attention.self.{n}.{kind}"] for n in ("query", "key", "value")] for i in range(cfg.num_hidden_layers)
                for kind in ("weight", "bias")]
        halves = [[opt.half(p) for p in t] for t in trip if t[0].dim() == 2]
        gouts = [torch.ones(sum(p.shape[0] for p in t), *t[0].shape[1:], device="cuda") for t in trip]

        def cats(backward):
            for _ in range(6):
                with torch.no_grad():
                    for t in halves:
                        torch.cat(t)
                if not backward:
                    with torch.no_grad():
                        for t in trip:
                            torch.cat(t)
                else:
                    torch.autograd.backward([torch.cat(t) for t in trip], gouts)

        for p in (q for t in trip for q in t):
            p.grad = torch.zeros_like(p)
        cat_ms = {}
        for name, bw in (("cat_forward", False), ("cat_forward_backward", True)):
            ts = []
            for i in range(13):
                sync()
                t0 = time.perf_counter()
                cats(bw)
                sync()
                if i >= 3:
                    ts.append((time.perf_counter() - t0) * 1e3)
            cat_ms[name] = median(ts)
        res["cat_ms"] = cat_ms
    except torch.cuda.OutOfMemoryError as e:
        res["oom"] = str(e).split("\n")[0][:200]
    print(json.dumps(res))


def run_child(B, steps):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(B), "--steps", str(steps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        print(f"B = {B}: exit {p.returncode}\n{p.stderr[-3000:]}", flush=True)
        sys.exit(1)  # the first failure stops the run: nothing more is started on the device
    r = json.loads(p.stdout.strip().split("\n")[-1])
    print(r, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step.md"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.steps)
    rows, notes = [], []
    for B in BATCHES:
        r = run_child(B, a.steps)
        for smaller in FALLBACK if "oom" in r else ():
            notes.append(f"{r['B']} samples per batch do not fit: {r['oom']}")
            r = run_child(smaller, a.steps)
            if "oom" not in r:
                notes.append(f"the largest batch of {(B,) + FALLBACK} that fits is {smaller}")
                break
        if "oom" in r:
            notes.append(f"{r['B']} samples per batch do not fit either: {r['oom']}")
            continue
        rows.append(r)
    gib = lambda b: f"{b / 2 ** 30:.2f}"  # noqa: E731
    lines = ["# One training step of the retriever", "",
             f"Command: `python scripts/measure/train_step_bench.py --steps {a.steps}` (roberta-base geometry, random weights, dropout 0.1, fp16 scores, "
             "dynamic loss scale; c1 / c2 / neg_1 / neg_2 padded to 300, q to 70, q_sp1 to 350, lengths uniform in [L / 2, L]; one MI355X; host clock around "
             f"work that ends in a synchronise, medians of {a.steps} steps after {WARMUP} warm-up steps; `whole` is the same step without the three inner "
             "synchronises).", "",
             "| samples | tokens | six forwards ms | loss ms | backward ms | optimizer ms | sum ms | whole step ms | samples / s |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        m = r["ms"]
        total = m["forward6"] + m["loss"] + m["backward"] + m["optimizer"]
        lines.append(f"| {r['B']} | {r['tokens']} | {m['forward6']:.1f} | {m['loss']:.2f} | {m['backward']:.1f} | {m['optimizer']:.2f} | {total:.1f} | {m['whole']:.1f} | "
                     f"{r['B'] / m['whole'] * 1e3:.1f} |")
    lines += ["", "Allocated memory (GiB, torch's allocator): before the step (masters, Adam's moments, fp16 copies, gradients), after the six forwards, "
              "their difference (what the graph keeps alive for the backward), and the peak of the step.", "",
              "| samples | before | after six forwards | kept for the backward | per encode (mean) | peak |", "|---|---|---|---|---|---|"]
    for r in rows:
        mm = r["mem"]
        kept = mm["after_forward"] - mm["before"]
        lines.append(f"| {r['B']} | {gib(mm['before'])} | {gib(mm['after_forward'])} | {gib(kept)} | {gib(kept / 6)} | {gib(mm['peak'])} |")
    lines += ["", "The head's backward alone (mdr_head_backward, dX + dW + db at [samples, 768] x [768, 768], device events, median of 50) and the per-encode "
              "torch.cat of the query / key / value leaves (the 6 x 12 concatenations of weights, biases and fp16 copies of one step; forward, and forward + "
              "backward = the split and the accumulation into the leaves' .grad), each as a share of the whole step.", "",
              "| samples | head backward ms | share of the step | cat forward ms | share | cat forward + backward ms | share |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        w, c = r["ms"]["whole"], r["cat_ms"]
        lines.append(f"| {r['B']} | {r['head_backward_ms']:.4f} | {r['head_backward_ms'] / w:.3%} | {c['cat_forward']:.2f} | {c['cat_forward'] / w:.2%} | "
                     f"{c['cat_forward_backward']:.2f} | {c['cat_forward_backward'] / w:.2%} |")
    lines += [""] + [f"- {n}" for n in notes] + ([""] if notes else [])
    lines.append(f"Steps skipped by the loss scaler during the runs: {', '.join(str(r['skipped_total']) + ' at ' + str(r['B']) for r in rows)} (the dynamic scale starts at "
                 "2^16 and halves on an overflow; a skipped step runs the same kernels).")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
