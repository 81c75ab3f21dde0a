"""Time the attention backward (mdr_attention_backward, include/mdr_attention_grad.h) against the backward of
torch.nn.functional.scaled_dot_product_attention on the same sequences padded to [B, 12, L, 64] fp16 with a key-padding mask, on the same device:

    python scripts/measure/attention_grad_bench.py [--out profiles/attention_grad_bench.md] [--iters 20]

Shapes (B, L) = (38, 300), (19, 350), (19, 70) -- the reference README's training command at 12 heads of 64 -- with lengths drawn uniformly in
[L / 2, L], and mode 3 (first query of each sequence) at (38, 300). The row pass and the column pass of mode 0 are also timed apart. Every
configuration runs in a child process of its own under a time limit; the first failure stops the run. Times are medians of `--iters` steps
after 3 warm-up steps, by device events around one step.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(38, 300), (19, 350), (19, 70)]
HEADS = 12
CHILD_LIMIT_S = 120


def child(B, L, which, iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import attention
    hidden = 64 * HEADS
    rng = np.random.default_rng([B, L])
    lens = rng.integers(L // 2, L + 1, size=B)
    cu_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T = int(cu_h[-1])
    qkv = torch.from_numpy(rng.standard_normal((T, 3 * hidden)).astype(np.float16)).cuda()
    cu = torch.from_numpy(cu_h).cuda()
    mode = attention.MODE_CLS if which == "hip3" else attention.MODE_ALL
    dctx = torch.from_numpy(rng.standard_normal((B if mode == attention.MODE_CLS else T, hidden)).astype(np.float16)).cuda()
    dqkv = torch.empty_like(qkv)

    if which == "torch":
        pad = torch.zeros((3, B, HEADS, L, 64), dtype=torch.float16, device="cuda")
        gpad = torch.zeros((B, HEADS, L, 64), dtype=torch.float16, device="cuda")
        mask = torch.zeros((B, 1, 1, L), dtype=torch.bool, device="cuda")
        for b, n in enumerate(lens):
            rows = qkv[int(cu_h[b]):int(cu_h[b + 1])]
            for i in range(3):
                pad[i, b, :, :n] = rows[:, i * hidden:(i + 1) * hidden].reshape(n, HEADS, 64).transpose(0, 1)
            gpad[b, :, :n] = dctx[int(cu_h[b]):int(cu_h[b + 1])].reshape(n, HEADS, 64).transpose(0, 1)
            mask[b, 0, 0, :n] = True
        q, k, v = (pad[i].clone().requires_grad_(True) for i in range(3))
        out = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask)  # the forward is outside the timed step

        def step():
            torch.autograd.grad(out, (q, k, v), gpad, retain_graph=True)
    elif which in ("hip", "hip3"):
        def step():
            attention.attention_backward(qkv, dctx, cu, HEADS, L, mode, out=dqkv)
    else:
        raise SystemExit(f"unknown leg {which}")

    times = []
    for i in range(3 + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(a.elapsed_time(b))
    times.sort()
    res = {"B": B, "L": L, "tokens": T, "which": which, "ms": times[len(times) // 2], "min_ms": times[0]}
    if which == "hip":  # the two passes apart, from the device's own kernel times
        from torch.profiler import ProfilerActivity, profile
        try:
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(iters):
                    step()
                torch.cuda.synchronize()
            for ev in prof.key_averages():
                if "attn_grad_kernel" in ev.key:
                    res["col_ms" if "Lb1" in ev.key or "<true>" in ev.key else "row_ms"] = ev.device_time_total / max(ev.count, 1) / 1000.0
        except Exception as e:  # the split is an extra: without a working profiler the table shows "-" there, the totals stand
            res["profiler_error"] = repr(e)[:200]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_grad_bench.md"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", nargs=3, default=None)
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), int(a.child[1]), a.child[2], a.iters)
    rows = []
    for B, L, legs in [(B, L, ("hip", "torch")) for B, L in SHAPES] + [(38, 300, ("hip3",))]:
        r = {}
        for which in legs:
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--child", str(B), str(L), which]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                print(f"B={B} L={L} {which}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
                sys.exit(1)  # the first failure stops the run: nothing more is started on the device
            r[which] = json.loads(p.stdout.strip().split("\n")[-1])
            print(r[which], flush=True)
        rows.append((B, L, r))
    fmt = lambda x: "-" if x is None else f"{x:.3f}"  # noqa: E731
    lines = ["# Attention backward: mdr_attention_backward against torch's scaled_dot_product_attention backward", "",
             "Command: `python scripts/measure/attention_grad_bench.py --iters %d` (12 heads of 64, fp16; lengths uniform in [L / 2, L]; torch on the same sequences "
             "padded to [B, 12, L, 64] with a key-padding mask, backward only; median of %d steps after 3 warm-up steps, device events; one MI355X). "
             "Row pass / column pass: the two kernels of mode 0 apart, from the profiler's kernel times." % (a.iters, a.iters),
             "", "| B | L | tokens | mode | HIP ms | row pass ms | column pass ms | torch ms | torch / HIP |", "|---|---|---|---|---|---|---|---|---|"]
    for B, L, r in rows:
        if "hip3" in r:
            lines.append(f"| {B} | {L} | {r['hip3']['tokens']} | 3 | {r['hip3']['ms']:.3f} | - | - | - | - |")
        else:
            h, t = r["hip"], r["torch"]
            lines.append(f"| {B} | {L} | {h['tokens']} | 0 | {h['ms']:.3f} | {fmt(h.get('row_ms'))} | {fmt(h.get('col_ms'))} | {t['ms']:.3f} | {t['ms'] / h['ms']:.2f} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
