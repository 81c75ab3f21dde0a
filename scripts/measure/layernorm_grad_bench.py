"""Time the LayerNorm backward (mdr_layernorm_backward, include/mdr_layernorm_grad.h) against torch.ops.aten.native_layer_norm_backward on the
same rows, on the same device:

    python scripts/measure/layernorm_grad_bench.py [--out profiles/layernorm_grad_bench.md] [--iters 20] [--reps 50]

H = 768. M = 8608 tokens (38 contexts with lengths uniform in [150, 300], the draw of scripts/measure/attention_grad_bench.py), M = 11400 =
38 x 300 (the largest token count one training batch of the reference README's command produces) and M = 38 (the CLS tail of the last layer).
The three operand combinations post_ln of csrc/mdr_encoder_trunk.inl issues, with the outputs a trunk pass needs of each:
    residual_fp32 = 0: in fp32 + res16, dy16 + dy2 fp16 -> dx16;   1: in fp32 + res32, dy16 + dy2 fp32 -> dx16, dx32;   2: in fp16 + res32, dy16 + dy2 fp32
    -> dx16, dx32;   dg and db always.
A call is a few tens of microseconds, so one timed step is `--reps` calls between two device events, divided by `--reps`; the figure is the
median of `--iters` steps after 3 warm-up steps. The calls go through the C ABI on preallocated buffers (what a trunk pass would do), torch's
through preallocated inputs. torch: x = in.float() + res.float() and dy = dy16.float() + dy2.float() (the adds it needs: it fuses neither),
native_layer_norm_backward in fp32 with the mean and rstd its forward would have saved, and dx.half() where the trunk needs dx16. The kernels
apart (ln_grad_kernel, grad_strand_reduce_kernel) from the profiler's kernel times. Bytes: what the call must move, every input row read once and
every output row written once (the [H] vectors and the partial sums left out); TB/s = bytes / call time, beside the ~6.3 TB/s a streaming
kernel reaches on this device. Every M runs in a child process of its own under a time limit; the first failure stops the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H = 768
TOKENS = [8608, 11400, 38]
# residual_fp32 -> (in, residual, dy2, outputs)
MODES = {0: ("f32", "f16", "f16", ("dx16",)), 1: ("f32", "f32", "f32", ("dx16", "dx32")), 2: ("f16", "f32", "f32", ("dx16", "dx32"))}
SIZE = {"f16": 2, "f32": 4, "dx16": 2, "dx32": 4}
CHILD_LIMIT_S = 150
STREAM_TBS = 6.3
KERNELS = {"main_kernel_ms": "ln_grad_kernel", "reduce_kernel_ms": "grad_strand_reduce_kernel"}


def bytes_moved(M, mode):
    tin, tres, tdy2, outs = MODES[mode]
    return M * H * (SIZE[tin] + SIZE[tres] + SIZE["f16"] + SIZE[tdy2] + sum(SIZE[o] for o in outs))


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


def child(M, iters, reps):
    import ctypes
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import _lib, layernorm
    L = layernorm.lib()
    dt = {"f16": torch.float16, "f32": torch.float32}
    rng = np.random.default_rng([M, H])
    draw = lambda scale=1.0: torch.from_numpy((scale * rng.standard_normal((M, H))).astype(np.float32)).cuda()  # noqa: E731
    g = torch.from_numpy((1.0 + 0.3 * rng.standard_normal(H)).astype(np.float32)).cuda()
    bias = torch.zeros(H, dtype=torch.float32, device="cuda")
    S, rpc = layernorm.backward_chunks(M, H)
    need = int(L.mdr_layernorm_backward_workspace_bytes(M, H, 3))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    dg, db = torch.zeros(H, dtype=torch.float32, device="cuda"), torch.zeros(H, dtype=torch.float32, device="cuda")
    stream = _lib.current_stream_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    out = []
    for mode, (tin, tres, tdy2, outs) in MODES.items():
        inp, res = draw().to(dt[tin]), draw().to(dt[tres])
        dy16, dy2 = draw().half(), draw().to(dt[tdy2])
        dx16 = torch.zeros((M, H), dtype=torch.float16, device="cuda")
        dx32 = torch.zeros((M, H), dtype=torch.float32, device="cuda") if "dx32" in outs else None
        res16, res32 = (res, None) if tres == "f16" else (None, res)

        def ours():
            _lib.check(L.mdr_layernorm_backward(p(inp), 1 if tin == "f16" else 0, p(res16), p(res32), p(dy16), p(dy2), 1 if tdy2 == "f32" else 0, M, None, H,
                                                p(g), 1e-5, p(dx16), p(dx32), p(dg), p(db), 0, p(ws), need, 0, stream))

        x32 = inp.float() + res.float()
        mean = x32.mean(-1, keepdim=True)
        rstd = (x32.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()

        def theirs():
            x = inp.float() + res.float()
            dy = dy16.float() + dy2.float()
            dx, tg, tb = torch.ops.aten.native_layer_norm_backward(dy, x, [H], mean, rstd, g, bias, [True, True, True])
            return dx.half(), dx, tg, tb

        def theirs_backward_only(x=x32, dy=dy16.float() + dy2.float()):
            return torch.ops.aten.native_layer_norm_backward(dy, x, [H], mean, rstd, g, bias, [True, True, True])

        r = {"M": M, "mode": mode, "S": S, "rows_per_chunk": rpc, "bytes": bytes_moved(M, mode)}
        r["call_ms"] = median_ms(ours, iters, reps)
        r["torch_ms"] = median_ms(theirs, iters, reps)
        r["torch_backward_only_ms"] = median_ms(theirs_backward_only, iters, reps)
        # the two agree (a sanity check of the comparison, not a test: tests/test_layernorm_grad_gpu.py holds the bound)
        tdx = theirs()[1]
        r["max_abs_diff_vs_torch"] = float((dx16.float() - tdx).abs().max())
        from torch.profiler import ProfilerActivity, profile
        try:  # the kernels apart, from the device's own kernel times
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(iters):
                    ours()
                torch.cuda.synchronize()
            for ev in prof.key_averages():
                for key, pat in sorted(KERNELS.items(), key=lambda kv: -len(kv[1])):
                    if pat in ev.key:
                        r[key] = r.get(key, 0.0) + ev.device_time_total / iters / 1000.0
                        break
        except Exception as e:  # the split is an extra: without a working profiler the table shows "-" there, the totals stand
            r["profiler_error"] = repr(e)[:200]
        out.append(r)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layernorm_grad_bench.md"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child(a.child, a.iters, a.reps)
    rows = []
    for M in TOKENS:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--reps", str(a.reps), "--child", str(M)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"M={M}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
            sys.exit(1)  # the first failure stops the run: nothing more is started on the device
        for r in json.loads(p.stdout.strip().split("\n")[-1]):
            print(r, flush=True)
            rows.append(r)
    f3 = lambda r, k: "-" if r.get(k) is None else f"{r[k]:.4f}"  # noqa: E731
    tbs = lambda r, k: "-" if r.get(k) is None else f"{r['bytes'] / (r[k] * 1e-3) / 1e12:.2f}"  # noqa: E731
    lines = ["# LayerNorm backward: mdr_layernorm_backward against torch.ops.aten.native_layer_norm_backward", "",
             "Command: `python scripts/measure/layernorm_grad_bench.py --iters %d --reps %d` (H = 768; one timed step is %d calls between two device events, "
             "divided by %d; median of %d steps after 3 warm-up steps; one MI355X). mode: the trunk's residual_fp32 (0: in fp32 + res16, dy16 + dy2 fp16 -> "
             "dx16; 1: in fp32 + res32, dy16 + dy2 fp32 -> dx16 + dx32; 2: in fp16 + res32, dy16 + dy2 fp32 -> dx16 + dx32), dg and db always. torch: the "
             "two adds it needs (x = in + res, dy = dy16 + dy2, in fp32), native_layer_norm_backward in fp32 with saved mean and rstd, and dx.half(); "
             "'torch backward only' leaves the adds and the cast out. MB: every input row read once and every output row written once. TB/s = MB / call "
             "time, beside the ~%.1f TB/s a streaming kernel reaches on this device. At M = 38 a call is shorter than the host takes to enqueue it: those "
             "rows measure the enqueue rate." % (a.iters, a.reps, a.reps, a.reps, a.iters, STREAM_TBS), "",
             "| M | mode | S | rows per chunk | MB | call ms | TB/s | main kernel ms | reduce kernel ms | kernels TB/s | torch ms | torch backward only ms | max abs dx diff vs torch |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        r["kernels_ms"] = None if r.get("main_kernel_ms") is None else r["main_kernel_ms"] + r.get("reduce_kernel_ms", 0.0)
        lines.append(f"| {r['M']} | {r['mode']} | {r['S']} | {r['rows_per_chunk']} | {r['bytes'] / 1e6:.1f} | {f3(r, 'call_ms')} | {tbs(r, 'call_ms')} | {f3(r, 'main_kernel_ms')} | "
                     f"{f3(r, 'reduce_kernel_ms')} | {tbs(r, 'kernels_ms')} | {f3(r, 'torch_ms')} | {f3(r, 'torch_backward_only_ms')} | {r['max_abs_diff_vs_torch']:.2e} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
