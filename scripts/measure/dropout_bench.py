"""Time dropout (include/mdr_dropout.h): the training attention forward and the backward that replays its mask against the same calls without
dropout and against torch's scaled_dot_product_attention(dropout_p=0.1), and the row kernel against a device copy:

    python scripts/measure/dropout_bench.py [--parent-lib PATH/TO/libmdrhip_parent.so] [--out profiles/dropout_bench.md] [--iters 30]

Attention: shapes (B, L) = (38, 300), (19, 350), (19, 70) at 12 heads of 64, lengths drawn uniformly in [L / 2, L] (the shapes of
profiles/attention_grad_bench.md), mode 0, and mode 3 at (38, 300); p = 0.1. The legs of one shape run in ONE child process, interleaved
round by round: the dropout forward and backward, the forward (mdr_test_attention) and backward (mdr_attention_backward) without dropout of
this build, and -- with --parent-lib, a build of the parent commit's sources -- the same two calls of that library on the same buffers (loaded
beside the product library; both use the process's one HIP runtime). torch: forward + backward of scaled_dot_product_attention(dropout_p=0.1)
on the same sequences padded to [B, 12, L, 64] with a key-padding mask. Rows: mdr_dropout_rows at [8608, 768], fp16, fp32 and fp32 with the
fp16 second output, against torch's copy_ of the same tensor (a vectorised device copy), in GB/s of the bytes the call must move. Times are
medians of `--iters` rounds after 3 warm-up rounds, by device events around one call. Every child runs under a time limit; the first failure
stops the run.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(38, 300, 0), (19, 350, 0), (19, 70, 0), (38, 300, 3)]
HEADS = 12
P, SEED, SITE = 0.1, 0x1234567890abcdef, 3
ROWS_SHAPE = (8608, 768)
CHILD_LIMIT_S = 150


def timed(legs, iters):
    """{name: median ms} of the callables in `legs`, interleaved round by round; 3 warm-up rounds."""
    import torch
    times = {k: [] for k in legs}
    for i in range(3 + iters):
        for name, step in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step()
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                times[name].append(a.elapsed_time(b))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def child_attention(B, L, mode, iters, parent_lib):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import _lib, attention, dropout
    from multihop_dense_retrieval_amd._lib import ptr
    hidden = 64 * HEADS
    rng = np.random.default_rng([B, L])
    lens = rng.integers(L // 2, L + 1, size=B)
    cu_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T = int(cu_h[-1])
    qkv = torch.from_numpy(rng.standard_normal((T, 3 * hidden)).astype(np.float16)).cuda()
    cu = torch.from_numpy(cu_h).cuda()
    out_rows = B if mode == 3 else T
    dctx = torch.from_numpy(rng.standard_normal((out_rows, hidden)).astype(np.float16)).cuda()
    ctx, dqkv = torch.zeros((out_rows, hidden), dtype=torch.float16, device="cuda"), torch.empty_like(qkv)
    thr = dropout.threshold(P)
    need = int(attention.lib().mdr_attention_backward_workspace_bytes(B, L, HEADS, mode))
    ws = _lib.workspace(need, qkv.device)
    stream = _lib.current_stream_ptr()

    def plain(lib):
        fwd = lambda: _lib.check(lib.mdr_test_attention(ptr(qkv), ptr(cu), None, B, L, hidden, HEADS, mode, ptr(ctx), 0, stream))  # noqa: E731
        bwd = lambda: _lib.check(lib.mdr_attention_backward(ptr(qkv), ptr(dctx), ptr(cu), B, L, hidden, HEADS, mode, ptr(dqkv), ptr(ws), need, 0, stream))  # noqa: E731
        return fwd, bwd

    legs = {"drop_fwd": lambda: attention.attention_dropout_forward(qkv, cu, HEADS, L, mode, thr, SEED, SITE, out=ctx),
            "drop_bwd": lambda: attention.attention_dropout_backward(qkv, dctx, cu, HEADS, L, mode, thr, SEED, SITE, out=dqkv)}
    legs["plain_fwd"], legs["plain_bwd"] = plain(attention.lib())
    if parent_lib:
        par = ctypes.CDLL(parent_lib)
        for name in ("mdr_test_attention", "mdr_attention_backward"):
            getattr(par, name).restype, getattr(par, name).argtypes = {**_lib._SIGNATURES, **attention.SIGNATURES}[name]
        legs["parent_fwd"], legs["parent_bwd"] = plain(par)
    if mode == 0:
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

        def torch_step():
            out = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=P)
            torch.autograd.grad(out, (q, k, v), gpad)
        legs["torch_fwd_bwd"] = torch_step
    res = {"B": B, "L": L, "tokens": T, "mode": mode}
    res.update(timed(legs, iters))
    print(json.dumps(res))


def child_rows(iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import _lib, dropout
    from multihop_dense_retrieval_amd._lib import ptr
    M, N = ROWS_SHAPE
    thr = dropout.threshold(P)
    L = dropout.lib()
    stream = _lib.current_stream_ptr()
    x32 = torch.from_numpy(np.random.default_rng(1).standard_normal((M, N)).astype(np.float32)).cuda()
    x16 = x32.half()
    y32, y16, c32, c16 = torch.empty_like(x32), torch.empty_like(x16), torch.empty_like(x32), torch.empty_like(x16)
    legs = {"rows_fp16": lambda: _lib.check(L.mdr_dropout_rows(ptr(x16), 1, None, M, None, N, thr, SEED, SITE, ptr(y16), None, 0, stream)),
            "rows_fp32": lambda: _lib.check(L.mdr_dropout_rows(ptr(x32), 0, None, M, None, N, thr, SEED, SITE, ptr(y32), None, 0, stream)),
            "rows_fp32_also16": lambda: _lib.check(L.mdr_dropout_rows(ptr(x32), 0, None, M, None, N, thr, SEED, SITE, ptr(y32), ptr(y16), 0, stream)),
            "copy_fp16": lambda: c16.copy_(x16), "copy_fp32": lambda: c32.copy_(x32)}
    res = {"ms": timed(legs, iters), "bytes": {"rows_fp16": 4 * M * N, "rows_fp32": 8 * M * N, "rows_fp32_also16": 10 * M * N, "copy_fp16": 4 * M * N,
                                              "copy_fp32": 8 * M * N}}
    print(json.dumps(res))


def run_child(args, env=None):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if p.returncode != 0:
        print(f"{args}: exit {p.returncode}\n{p.stderr[-3000:]}", flush=True)
        sys.exit(1)  # the first failure stops the run: nothing more is started on the device
    r = json.loads(p.stdout.strip().split("\n")[-1])
    print(r, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropout_bench.md"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's sources (build.py --out=... in a checkout of it)")
    ap.add_argument("--child", nargs="+", default=None)
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None
    if a.child:
        if a.child[0] == "rows":
            return child_rows(a.iters)
        return child_attention(int(a.child[0]), int(a.child[1]), int(a.child[2]), a.iters, parent)
    if parent and not os.path.exists(parent):
        sys.exit(f"no such library: {parent}")
    common = ["--iters", str(a.iters)] + (["--parent-lib", parent] if parent else [])
    att = [run_child(common + ["--child", str(B), str(L), str(mode)]) for B, L, mode in SHAPES]
    rows = run_child(common + ["--child", "rows"])
    base = "parent" if parent else "plain"
    fmt = lambda r, k: "-" if k not in r else f"{r[k]:.3f}"  # noqa: E731
    lines = ["# Dropout: the training attention forward and backward, and the row kernel", "",
             f"Command: `python scripts/measure/dropout_bench.py --iters {a.iters}{' --parent-lib <the parent commit built with build.py --out=...>' if parent else ''}` "
             f"(12 heads of 64, fp16, p = 0.1 which draws 26 / 256; lengths uniform in [L / 2, L]; median of {a.iters} rounds after 3 warm-up rounds, device "
             "events around one call, the legs of a row interleaved in one process; one MI355X). parent: the forward (mdr_test_attention) and "
             "mdr_attention_backward of the parent commit's library on the same buffers; no dropout: the same calls of this build; torch: "
             "scaled_dot_product_attention(dropout_p=0.1) forward + backward on the padded batch.", "",
             "| B | L | tokens | mode | dropout fwd ms | dropout bwd ms | no dropout fwd ms | no dropout bwd ms | parent fwd ms | parent bwd ms | fwd / "
             f"{base} | bwd / {base} | torch fwd + bwd ms | torch / (dropout fwd + bwd) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in att:
        both = r["drop_fwd"] + r["drop_bwd"]
        lines.append(f"| {r['B']} | {r['L']} | {r['tokens']} | {r['mode']} | {r['drop_fwd']:.3f} | {r['drop_bwd']:.3f} | {r['plain_fwd']:.3f} | {r['plain_bwd']:.3f} | "
                     f"{fmt(r, 'parent_fwd')} | {fmt(r, 'parent_bwd')} | {r['drop_fwd'] / r[base + '_fwd']:.2f} | {r['drop_bwd'] / r[base + '_bwd']:.2f} | "
                     f"{fmt(r, 'torch_fwd_bwd')} | {'-' if 'torch_fwd_bwd' not in r else format(r['torch_fwd_bwd'] / both, '.2f')} |")
    lines += ["", f"Rows at [{ROWS_SHAPE[0]}, {ROWS_SHAPE[1]}] (GB/s of the bytes the call must read and write):", "", "| call | ms | GB/s |", "|---|---|---|"]
    for k, ms in rows["ms"].items():
        lines.append(f"| {k} | {ms:.4f} | {rows['bytes'][k] / ms / 1e6:.0f} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
