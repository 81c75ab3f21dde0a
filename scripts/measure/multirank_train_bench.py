"""Time one retriever training step on 1, 2, 4 and 8 ranks (multihop_dense_retrieval_amd/dist.py) and write
profiles/multirank_train.md:

    python scripts/measure/multirank_train_bench.py [--out profiles/multirank_train.md] [--steps 5] [--ranks 1,2,4,8] [--batch 150]
    python scripts/measure/multirank_train_bench.py --one-rank-of PATH      # the one-rank row of another checkout (the parent commit), JSON on stdout

The batch of scripts/measure/train_step_bench.py: roberta-base geometry with random weights, dropout 0.1, --fp16 scores, the dynamic loss
scale, 150 samples, c1 / c2 / neg_1 / neg_2 padded to 300, q to 70, q_sp1 to 350, lengths uniform in [L / 2, L]. N ranks are N child processes
started here with RANK / WORLD_SIZE / LOCAL_RANK on a loopback address, each under a time limit; the first failure stops the run. With at
least N visible devices every rank has its own and the transport is nccl (RCCL); with fewer, all ranks share device 0 over gloo (the
rehearsal mode: the ranks then queue behind each other on one card and the flat buffer crosses the host, so such a row says what the
rehearsal costs, not what N devices would give). The profile says which rows are which.

A step is split by host clocks around work that ends in a device synchronise: the six forwards of this rank's rows, the six gathers, the
loss and the backward, then exchange, mdr_rank_sum, publish and the optimizer step; `whole` is train_step + reduce() + opt.step() with one
synchronise at the end. Rank 0's medians of --steps steps after 2 warm-up steps. The one-rank row takes no world (the code path of a run
without a launcher) and --one-rank-of measures the same row from another checkout's package in the same session, so that the parent commit
can be put beside it. The kernel alone: mdr_rank_sum over N rows of a roberta-base segment (device events, median of 20) as bytes read and
written per second, next to a device-to-device copy_ of the same number of bytes on the same card.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LENS = {"q": 70, "q_sp": 350, "c1": 300, "c2": 300, "neg1": 300, "neg2": 300}
CHILD_LIMIT_S = 600
WARMUP = 2


def median(v):
    return sorted(v)[len(v) // 2]


def make_batch(B, vocab):
    import numpy as np
    import torch
    rng = np.random.default_rng(B)
    batch = {}
    for key, L in LENS.items():
        lens = rng.integers(L // 2, L + 1, size=B)
        ids = rng.integers(3, vocab, size=(B, L))
        mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
        ids = np.where(mask == 1, ids, 0)
        ids[:, 0] = 0
        batch[f"{key}_input_ids"], batch[f"{key}_mask"] = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    return batch


def child(a):
    """One rank. `a.root` is the checkout whose package is measured."""
    import types
    import torch
    sys.path.insert(0, a.root)
    from multihop_dense_retrieval_amd import criterions, retriever, train
    rank, N = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(0 if a.share_gpu else int(os.environ.get("LOCAL_RANK", "0")))
    world = bucket = None
    torch.manual_seed(0)  # the same weights on every rank
    cfg = retriever.RobertaConfig()
    cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = 0.1, 0.1
    args = types.SimpleNamespace(learning_rate=2e-5, adam_epsilon=1e-8, max_grad_norm=2.0, weight_decay=0.0, gradient_accumulation_steps=1, fp16=True,
                                 momentum=False)
    model = train.TrainableRetriever(cfg, args).cuda().train()
    opt = train.optimizer_for(model, args)
    if N > 1:
        from datetime import timedelta
        import torch.distributed
        from multihop_dense_retrieval_amd import dist
        torch.distributed.init_process_group("gloo" if a.share_gpu else "nccl", timeout=timedelta(seconds=CHILD_LIMIT_S))
        world = dist.TorchWorld()
        bucket = dist.GradBucket(model.parameters(), world)
    batch = make_batch(a.batch, cfg.vocab_size)
    sync = torch.cuda.synchronize
    names = ("forward6", "gather", "loss_backward", "exchange", "rank_sum", "publish", "optimizer", "whole")
    parts = {k: [] for k in names}
    for i in range(WARMUP + a.steps):
        sync()
        t = [time.perf_counter()]

        def mark():
            sync()
            t.append(time.perf_counter())

        if world is None:
            out = model(batch, seed=100 + i, half=opt.half)
            mark()
            mark()
            opt.scale_loss(criterions.mhop_loss_outputs(out, args)).backward()
            mark()
            mark(), mark(), mark()
        else:
            bounds = dist.slice_bounds(a.batch, N)
            lo, hi = bounds[rank]
            local = {k: v[lo:hi] for k, v in batch.items()}
            out = model(local, seed=dist.rank_seed(100 + i, rank), half=opt.half)
            mark()
            full = {n: dist.gather_with_grad(world, out[n], bounds) for n in train.ENCODE_INDEX}
            mark()
            opt.scale_loss(criterions.mhop_loss_outputs(full, args)).backward()
            mark()
            recv = world.exchange(bucket.flat)
            mark()
            dist.rank_sum(recv, bucket.mine)
            mark()
            world.publish(bucket.mine, bucket.flat)
            mark()
            del full, recv
        del out
        opt.step()
        mark()
        extra = {"world": world, "bucket": bucket} if world is not None else {}
        train.train_step(model, batch, args, opt, 200 + i, **extra)
        if bucket is not None:
            bucket.reduce()
        opt.step()
        mark()
        if i >= WARMUP:
            for k, d in zip(names, (t[j + 1] - t[j] for j in range(len(names)))):
                parts[k].append(d * 1e3)
    res = {"ranks": N, "B": a.batch, "transport": "none" if N == 1 else ("gloo, one shared device" if a.share_gpu else "nccl, a device per rank"),
           "ms": {k: median(v) for k, v in parts.items()}, "skipped_total": opt.read_state()["skipped_total"],
           "peak_gib": torch.cuda.max_memory_allocated() / 2 ** 30}
    if world is not None:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if rank == 0:
        print(json.dumps(res), flush=True)


def kernel_child(a):
    import torch
    sys.path.insert(0, a.root)
    from multihop_dense_retrieval_amd import dist, retriever
    total = sum(int(torch.Size(s).numel()) for k, s in retriever.expected_state_dict_shapes(retriever.RobertaConfig()).items() if "pooler" not in k)
    rows = []

    def timed(fn):
        ts = []
        for i in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ts.append(e0.elapsed_time(e1))
        return median(ts)

    for N in (2, 4, 8):
        _, S, _ = dist.flat_layout([total], N)
        recv, out = torch.randn(N, S, device="cuda"), torch.empty(S, device="cuda")
        ms = timed(lambda: dist.rank_sum(recv, out))
        nbytes = (N + 1) * S * 4
        src = torch.empty(nbytes // 8, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        copy_ms = timed(lambda: dst.copy_(src))
        rows.append({"ranks": N, "segment": S, "ms": ms, "bytes": nbytes, "copy_ms": copy_ms, "copy_bytes": 2 * src.numel() * 4})
        del recv, out, src, dst
    print(json.dumps({"total": total, "rows": rows}), flush=True)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(N, a, devices, root=ROOT):
    share = N > devices
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", "--root", root, "--steps", str(a.steps),
           "--batch", str(a.batch)] + (["--share-gpu"] if share else [])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multirank_train.md"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=150)
    ap.add_argument("--ranks", default="1,2,4,8")
    ap.add_argument("--one-rank-of", default=None)
    ap.add_argument("--parent-json", default=None, help="the JSON line --one-rank-of printed for the parent commit in this session")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--share-gpu", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.kernel:
        return kernel_child(a)
    import torch
    devices = torch.cuda.device_count()
    if a.one_rank_of is not None:
        return run_ranks(1, a, devices, root=os.path.abspath(a.one_rank_of))
    rows = [run_ranks(int(n), a, devices) for n in a.ranks.split(",")]
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--kernel"], capture_output=True, text=True)
    if p.returncode != 0:
        print(p.stderr[-3000:])
        sys.exit(1)
    kern = json.loads(p.stdout.strip().split("\n")[-1])
    parent = json.loads(open(a.parent_json).read().strip().split("\n")[-1].replace("'", '"')) if a.parent_json else None
    lines = ["# One retriever training step on several ranks", "",
             f"Command: `python scripts/measure/multirank_train_bench.py --steps {a.steps} --batch {a.batch} --ranks {a.ranks}` ({devices} visible MI355X; roberta-base geometry, "
             "random weights, dropout 0.1, fp16 scores, dynamic loss scale; the batch of `profiles/train_step.md`; rank 0's host clocks around work that ends in a "
             f"synchronise, medians of {a.steps} steps after {WARMUP} warm-up steps; `whole` is the same step with one synchronise at the end).", "",
             "| ranks | transport | six forwards ms | gathers ms | loss + backward ms | exchange ms | mdr_rank_sum ms | publish ms | optimizer ms | whole step ms | samples / s | peak GiB |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows + ([dict(parent, transport="none (the parent commit, same session)")] if parent else []):
        m = r["ms"]
        lines.append(f"| {r['ranks']} | {r['transport']} | {m['forward6']:.1f} | {m['gather']:.2f} | {m['loss_backward']:.1f} | {m['exchange']:.2f} | {m['rank_sum']:.3f} | "
                     f"{m['publish']:.2f} | {m['optimizer']:.2f} | {m['whole']:.1f} | {r['B'] / m['whole'] * 1e3:.1f} | {r['peak_gib']:.2f} |")
    lines += ["", f"The kernel alone, over the rows of one segment of the {kern['total']} trainable fp32 values (device events, median of 20), next to a device-to-device "
              "`copy_` that moves the same number of bytes (read + written) on the same card:", "",
              "| ranks | segment floats | mdr_rank_sum ms | bytes read + written | GB/s | copy_ ms | copy GB/s | kernel / copy rate |", "|---|---|---|---|---|---|---|---|"]
    for k in kern["rows"]:
        rate, copy = k["bytes"] / k["ms"] / 1e6, k["copy_bytes"] / k["copy_ms"] / 1e6
        lines.append(f"| {k['ranks']} | {k['segment']} | {k['ms']:.3f} | {k['bytes']} | {rate:.0f} | {k['copy_ms']:.3f} | {copy:.0f} | {rate / copy:.2f} |")
    lines += ["", f"Steps skipped by the loss scaler during the runs: {', '.join(str(r['skipped_total']) + ' at ' + str(r['ranks']) + ' ranks' for r in rows)}."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
