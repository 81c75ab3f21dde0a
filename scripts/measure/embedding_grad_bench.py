"""Time the embedding backward (include/mdr_embedding_grad.h: mdr_embedding_plan, mdr_embedding_scatter, mdr_embedding_backward) against
torch's own composition on the same tensors, on the same device:

    python scripts/measure/embedding_grad_bench.py [--out profiles/embedding_grad_bench.md] [--iters 20] [--reps 50]

H = 768, vocab 50265, max_pos 514, pad_row 1. Tokens: 8608 (38 sequences with lengths uniform in [150, 300], scaled to that sum), 11400 =
38 x 300 and 38 (one short sequence: the launch floor); cap = the forward's B * L. The ids are a seeded Zipf-like draw (rank r with
probability ~ 1 / r over the vocabulary) with <s> (0) first and </s> (2) last in every sequence; position ids 2, 3, ... as RoBERTa counts
them. The seed, the number of distinct ids and the longest segment are printed.

Timed: the plan alone (it is enqueued at forward time), the scatter alone (dword, dpos and dtype0 from a given d, accumulate = 1), the whole
call (all five outputs, dy16 + fp32 dy2) with accumulate = 1 -- the training path: six forwards accumulate into one buffer -- and with
accumulate = 0, which zeroes 154 MB first as torch's dense gradient does. torch: dy = dy16.float() + dy2,
aten.native_layer_norm_backward on a materialised x with saved mean and rstd, aten.embedding_dense_backward for both tables (each returns a
fresh dense table) and d.sum(0). One timed step is `--reps` calls between two device events, divided by `--reps`; the figure is the median
of `--iters` steps after 3 warm-up steps. The kernels apart from the profiler's kernel times. Scatter bytes: every d row read three times
(once per table, once for dtype0) and every table row that owns a segment read and written once; TB/s beside the ~6.3 TB/s a streaming
kernel reaches on this device. Every token count runs in a child process of its own under a time limit; the first failure stops the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, VOCAB, MAX_POS, PAD = 768, 50265, 514, 1
TOKENS = [8608, 11400, 38]
SEED = 20240
CHILD_LIMIT_S = 200
STREAM_TBS = 6.3
KERNELS = {"keys_ms": "emb_keys_kernel", "rank_ms": "emb_rank_kernel", "segments_ms": "emb_segments_kernel", "ln_grad_ms": "emb_ln_grad_kernel",
           "reduce_ms": "grad_strand_reduce_kernel", "scatter_kernel_ms": "emb_scatter_kernel", "colsum_ms": "emb_colsum_kernel"}


def lengths(tokens, rng):
    if tokens == 38:
        return [38]
    if tokens == 11400:
        return [300] * 38
    n = rng.integers(150, 301, 38).astype(float)
    n = (n * tokens / n.sum()).astype(int)
    n[0] += tokens - n.sum()
    return [int(v) for v in n]


def draw_batch(tokens):
    """-> ids int64 [B, L] (pad 1 behind every sequence), tok_src, tok_pid int32 [B L], total"""
    import numpy as np
    rng = np.random.default_rng([SEED, tokens])
    lens = lengths(tokens, rng)
    B, L = len(lens), max(lens)
    ids = np.full((B, L), PAD, np.int64)
    src, pid = [], []
    for b, n in enumerate(lens):
        r = np.exp(rng.random(n) * np.log(VOCAB - 4)).astype(np.int64)  # rank r with probability ~ 1 / r
        ids[b, :n] = 3 + r
        ids[b, 0], ids[b, n - 1] = 0, 2
        src += [b * L + j for j in range(n)]
        pid += [j + 1 + PAD for j in range(n)]
    total, cap = len(src), B * L
    tok_src, tok_pid = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    tok_src[:total], tok_pid[:total] = src, pid
    return ids, tok_src, tok_pid, total


def median_ms(step, iters, reps):
    import torch
    times = []
    for i in range(3 + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            step()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(a.elapsed_time(b) / reps)
    times.sort()
    return times[len(times) // 2]


def child(tokens, iters, reps):
    import ctypes
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import _lib, embedding
    L = embedding.lib()
    ids_h, src_h, pid_h, total = draw_batch(tokens)
    cap = len(src_h)
    wid_h = np.clip(ids_h.reshape(-1)[src_h[:total]], 0, VOCAB - 1)
    counts = np.bincount(wid_h)
    rng = np.random.default_rng([SEED, tokens, H])
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ids, src, pid, tot = cuda(ids_h), cuda(src_h), cuda(pid_h), torch.tensor([total], dtype=torch.int32, device="cuda")
    word = cuda((0.1 * rng.standard_normal((VOCAB, H))).astype(np.float32))
    pos = cuda((0.1 * rng.standard_normal((MAX_POS, H))).astype(np.float32))
    type0 = cuda((0.1 * rng.standard_normal(H)).astype(np.float32))
    g = cuda((1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32))
    bias = torch.zeros(H, dtype=torch.float32, device="cuda")
    dy16 = cuda(rng.standard_normal((cap, H)).astype(np.float16))
    dy2 = cuda(rng.standard_normal((cap, H)).astype(np.float32))
    dword, dpos = torch.zeros_like(word), torch.zeros_like(pos)
    dtype0, dg, db = (torch.zeros(H, dtype=torch.float32, device="cuda") for _ in range(3))
    d32 = torch.zeros((cap, H), dtype=torch.float32, device="cuda")
    plan_bytes = int(L.mdr_embedding_plan_bytes(cap))
    plan = torch.zeros(plan_bytes // 4, dtype=torch.int32, device="cuda")
    sneed, bneed = int(L.mdr_embedding_scatter_workspace_bytes(cap, H)), int(L.mdr_embedding_backward_workspace_bytes(cap, H))
    ws = torch.empty(bneed, dtype=torch.uint8, device="cuda")
    stream = _lib.current_stream_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731

    def plan_call():
        _lib.check(L.mdr_embedding_plan(p(ids), p(src), p(pid), p(tot), cap, VOCAB, MAX_POS, PAD, p(plan), plan_bytes, 0, stream))

    def scatter_call():
        _lib.check(L.mdr_embedding_scatter(p(d32), p(plan), cap, H, VOCAB, MAX_POS, p(dword), p(dpos), p(dtype0), 1, p(ws), sneed, 0, stream))

    def backward_call(accumulate=1):
        _lib.check(L.mdr_embedding_backward(p(ids), p(src), p(pid), p(tot), cap, p(word), p(pos), p(type0), p(g), H, VOCAB, MAX_POS, 1e-5, p(dy16), p(dy2), 1,
                                            p(plan), p(dword), p(dpos), p(dtype0), p(dg), p(db), None, accumulate, p(ws), bneed, 0, stream))

    wid = cuda(wid_h)
    prow = cuda(np.minimum(pid_h[:total], MAX_POS - 1).astype(np.int64))
    x = (word[wid] + pos[prow]) + type0
    mean = x.mean(-1, keepdim=True)
    rstd = (x.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()

    def theirs():
        dy = dy16[:total].float() + dy2[:total]
        d, tg, tb = torch.ops.aten.native_layer_norm_backward(dy, x, [H], mean, rstd, g, bias, [True, True, True])
        return (torch.ops.aten.embedding_dense_backward(d, wid, VOCAB, PAD, False), torch.ops.aten.embedding_dense_backward(d, prow, MAX_POS, PAD, False),
                d.sum(0), tg, tb, d)

    plan_call()
    torch.cuda.synchronize()
    lay = embedding.plan_layout(cap)
    head = plan[:8].cpu().numpy()
    nseg_w, nseg_p = int(head[2]), int(head[3])
    r = {"tokens": total, "cap": cap, "seed": SEED, "distinct_ids": int((counts > 0).sum()), "longest_segment": int(counts.max()), "segments_word": nseg_w,
         "segments_pos": nseg_p, "scatter_bytes": 3 * total * H * 4 + 2 * (nseg_w + nseg_p) * H * 4}
    assert nseg_w == r["distinct_ids"] and int(plan[lay["word"]["seg_start"] + nseg_w]) == total
    # the two agree (a sanity check of the comparison, not a test: tests/test_embedding_grad_gpu.py holds the bound)
    for t in (dword, dpos, dtype0, dg, db):
        t.zero_()
    backward_call(0)
    tw, tp, tt, tg, tb, td = theirs()
    torch.cuda.synchronize()
    r["max_abs_diff_vs_torch"] = max(float((a - b).abs().max()) for a, b in ((dword, tw), (dpos, tp), (dtype0, tt), (dg, tg), (db, tb)))
    d32[:total] = td
    r["plan_ms"] = median_ms(plan_call, iters, reps)
    r["scatter_ms"] = median_ms(scatter_call, iters, reps)
    r["call_ms"] = median_ms(backward_call, iters, reps)
    r["call_overwrite_ms"] = median_ms(lambda: backward_call(0), iters, reps)
    r["torch_ms"] = median_ms(theirs, iters, reps)
    from torch.profiler import ProfilerActivity, profile
    try:  # the kernels apart, from the device's own kernel times
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                plan_call()
                backward_call()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            for key, pat in KERNELS.items():
                if pat in ev.key:
                    r[key] = r.get(key, 0.0) + ev.device_time_total / iters / 1000.0
                    break
    except Exception as e:  # the split is an extra: without a working profiler the table shows "-" there, the totals stand
        r["profiler_error"] = repr(e)[:200]
    print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embedding_grad_bench.md"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.iters, a.reps)
    rows = []
    for tokens in TOKENS:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--reps", str(a.reps), "--child", str(tokens)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"tokens={tokens}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
            sys.exit(1)  # the first failure stops the run: nothing more is started on the device
        r = json.loads(p.stdout.strip().split("\n")[-1])
        print(r, flush=True)
        rows.append(r)
    f4 = lambda r, k: "-" if r.get(k) is None else f"{r[k]:.4f}"  # noqa: E731
    lines = ["# Embedding backward: mdr_embedding_plan / mdr_embedding_scatter / mdr_embedding_backward against torch's composition", "",
             "Command: `python scripts/measure/embedding_grad_bench.py --iters %d --reps %d` (H = 768, vocab 50265, max_pos 514, pad_row 1; one timed step is %d "
             "calls between two device events, divided by %d; median of %d steps after 3 warm-up steps; one MI355X). ids: seeded Zipf-like draw (seed %d), "
             "<s> and </s> in every sequence. plan: mdr_embedding_plan alone (enqueued at forward time). scatter: dword, dpos and dtype0 from a given d, "
             "accumulate = 1. call: mdr_embedding_backward, all five outputs, dy16 + fp32 dy2, accumulate = 1 (the training path); call overwrite: "
             "accumulate = 0, which zeroes the 154 MB word table first. torch: dy16.float() + dy2, aten.native_layer_norm_backward with saved mean and "
             "rstd on a materialised x, aten.embedding_dense_backward for both tables (fresh dense tables) and d.sum(0). scatter MB: every d row read three "
             "times and every table row that owns a segment read and written; TB/s = MB / scatter time, beside the ~%.1f TB/s a streaming kernel reaches on "
             "this device. At 38 tokens a call is shorter than the host takes to enqueue its launches: that row measures the enqueue rate."
             % (a.iters, a.reps, a.reps, a.reps, a.iters, SEED, STREAM_TBS), "",
             "| tokens | cap | distinct ids | longest segment | position segments | plan ms | scatter ms | scatter MB | scatter TB/s | call ms | call overwrite ms | torch ms | "
             "torch / call | torch / call overwrite | max abs diff vs torch |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['tokens']} | {r['cap']} | {r['distinct_ids']} | {r['longest_segment']} | {r['segments_pos']} | {f4(r, 'plan_ms')} | {f4(r, 'scatter_ms')} | "
                     f"{r['scatter_bytes'] / 1e6:.1f} | {r['scatter_bytes'] / (r['scatter_ms'] * 1e-3) / 1e12:.2f} | {f4(r, 'call_ms')} | {f4(r, 'call_overwrite_ms')} | "
                     f"{f4(r, 'torch_ms')} | {r['torch_ms'] / r['call_ms']:.2f} | {r['torch_ms'] / r['call_overwrite_ms']:.2f} | {r['max_abs_diff_vs_torch']:.2e} |")
    lines += ["", "Kernel times of one plan and one call (accumulate = 1), from the profiler, ms:", "",
              "| tokens | emb_keys | emb_rank | emb_segments | emb_ln_grad | grad_strand_reduce | emb_scatter |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['tokens']} | " + " | ".join(f4(r, k) for k in ("keys_ms", "rank_ms", "segments_ms", "ln_grad_ms", "reduce_ms", "scatter_kernel_ms")) + " |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
