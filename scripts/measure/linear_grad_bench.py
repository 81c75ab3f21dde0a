"""Time the Linear backward (mdr_linear_backward, include/mdr_linear_grad.h) piece by piece against torch's fp16 matrix products on the same
tensors, on the same device:

    python scripts/measure/linear_grad_bench.py [--out profiles/linear_grad_bench.md] [--iters 20]

Shapes: the four Linears of roberta-base, (N, K) = (2304, 768) QKV, (768, 768) out-projection, (3072, 768) FFN1, (768, 3072) FFN2, each at
M = 8608 tokens (38 contexts with lengths uniform in [150, 300], the draw of scripts/measure/attention_grad_bench.py) and at M = 11400 =
38 x 300, the largest token count one training batch of the reference README's command produces (19 samples per device, two contexts each,
--max_c_len 300). Per shape: the dX call (transpose + the forward GEMM on W^T), the dW call (tile kernel + reduction), the db call and the
call that computes all three, each a median of `--iters` steps after 3 warm-up steps by device events around one step; the kernels apart
(transpose, dgrad GEMM, wgrad tiles, reduction, column sums, gelu') from the profiler's kernel times; FFN1 also with the GELU path. torch:
dY @ W, dY.t() @ X and dY.sum(0) in fp16. Every shape runs in a child process of its own under a time limit; the first failure stops the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LINEARS = [("QKV", 2304, 768), ("out-proj", 768, 768), ("FFN1", 3072, 768), ("FFN2", 768, 3072)]
TOKENS = [8608, 11400]
CHILD_LIMIT_S = 120
KERNELS = {"transpose_ms": "lg_transpose_kernel", "wgrad_tiles_ms": "lg_wgrad_kernel", "reduce_ms": "lg_reduce_kernel", "colsum_ms": "lg_colsum_kernel",
           "gelu_grad_ms": "lg_gelu_grad_kernel", "dgrad_gemm_ms": "gemm_"}


def median_ms(step, iters):
    import torch
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
    return times[len(times) // 2]


def child(N, K, M, iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import linear
    rng = np.random.default_rng([N, K, M])
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float16)).cuda()
    w = torch.from_numpy((0.02 * rng.standard_normal((N, K))).astype(np.float16)).cuda()
    dy = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float16)).cuda()
    pre = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float16)).cuda()
    dw = torch.zeros((N, K), dtype=torch.float32, device="cuda")
    db = torch.zeros(N, dtype=torch.float32, device="cuda")
    S, rpc = linear.backward_chunks(M, N, K)
    res = {"N": N, "K": K, "M": M, "S": S, "rows_per_chunk": rpc}
    legs = {
        "dx_ms": lambda: linear.linear_backward(x, w, dy, need_dx=True),
        "dw_ms": lambda: linear.linear_backward(x, w, dy, need_dx=False, dw=dw),
        "db_ms": lambda: linear.linear_backward(x, w, dy, need_dx=False, db=db),
        "all_ms": lambda: linear.linear_backward(x, w, dy, need_dx=True, dw=dw, db=db),
        "all_gelu_ms": lambda: linear.linear_backward(x, w, dy, pre, need_dx=True, dw=dw, db=db),
        "torch_dx_ms": lambda: dy @ w,
        "torch_dw_ms": lambda: dy.t() @ x,
        "torch_db_ms": lambda: dy.sum(0),
    }
    for name, step in legs.items():
        res[name] = median_ms(step, iters)
    from torch.profiler import ProfilerActivity, profile
    try:  # the kernels apart, from the device's own kernel times
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                legs["all_gelu_ms"]()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            for key, pat in KERNELS.items():
                if pat in ev.key:
                    res[key] = res.get(key, 0.0) + ev.device_time_total / iters / 1000.0
    except Exception as e:  # the split is an extra: without a working profiler the table shows "-" there, the totals stand
        res["profiler_error"] = repr(e)[:200]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_grad_bench.md"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", nargs=3, default=None)
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), int(a.child[1]), int(a.child[2]), a.iters)
    rows = []
    for name, N, K in LINEARS:
        for M in TOKENS:
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--child", str(N), str(K), str(M)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                print(f"{name} M={M}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
                sys.exit(1)  # the first failure stops the run: nothing more is started on the device
            r = json.loads(p.stdout.strip().split("\n")[-1])
            print(r, flush=True)
            rows.append((name, r))
    f3 = lambda r, k: "-" if r.get(k) is None else f"{r[k]:.3f}"  # noqa: E731
    lines = ["# Linear backward: mdr_linear_backward against torch's fp16 matrix products", "",
             "Command: `python scripts/measure/linear_grad_bench.py --iters %d` (fp16 operands, fp32 dW and db; median of %d steps after 3 warm-up steps, device "
             "events around one call, so the call columns include the launch gaps between a call's kernels; one MI355X). torch: `dY @ W`, `dY.t() @ X`, "
             "`dY.sum(0)` in fp16 on the same tensors. S: chunks of the token rows the weight-gradient kernel splits into." % (a.iters, a.iters), "",
             "Calls (ms):", "",
             "| Linear | N | K | M | S | dX call | torch dY @ W | dW call | torch dY.t() @ X | db call | torch dY.sum(0) | all three | all three + gelu' |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in rows:
        lines.append(f"| {name} | {r['N']} | {r['K']} | {r['M']} | {r['S']} | {f3(r, 'dx_ms')} | {f3(r, 'torch_dx_ms')} | {f3(r, 'dw_ms')} | {f3(r, 'torch_dw_ms')} | "
                     f"{f3(r, 'db_ms')} | {f3(r, 'torch_db_ms')} | {f3(r, 'all_ms')} | {f3(r, 'all_gelu_ms')} |")
    lines += ["", "Kernels of the call with all three outputs and gelu' (ms, profiler kernel times):", "",
              "| Linear | M | transpose | dgrad GEMM | wgrad tiles | wgrad reduction + db reduction | column sums | gelu' |", "|---|---|---|---|---|---|---|---|"]
    for name, r in rows:
        lines.append(f"| {name} | {r['M']} | {f3(r, 'transpose_ms')} | {f3(r, 'dgrad_gemm_ms')} | {f3(r, 'wgrad_tiles_ms')} | {f3(r, 'reduce_ms')} | {f3(r, 'colsum_ms')} | "
                     f"{f3(r, 'gelu_grad_ms')} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
