"""Cost of one dev-set MRR batch (scripts/train_mhop.py --do_predict) on one MI355X at roberta-base geometry, for B in {150, 1000, 3000}:

    python scripts/measure/mhop_eval_bench.py [--batches 150,1000,3000] [--runs 20] [--timeout 600] [--out profiles/mhop_eval_bench.md]

Per B: the six forwards (RobertaRetriever.forward on a synthetic mhop_collate batch: questions of 20-30 tokens, q_sp of 150-250, passages of
100-300, right-padded with 0), mdr_inbatch_rank in both modes, and the reference composition of mhop_eval on the same device -- torch.mm,
torch.bmm, the masked_fill round trip, two argsorts of each [B, 2B + 2] matrix and the gather of the targets' ranks (without the reference's
host loop over .item()) -- on fp32 and on fp16 operands. HIP events, after warm-up, the median of --runs runs (the forwards: of max(3, runs / 5)
runs). Random weights and random embeddings: only the shapes matter. Each B runs in its own child process under its own timeout, and the parent
stops at the first child that fails; one JSON line per B, then the markdown table.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, runs, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def torch_composition(o, half):
    import torch
    c = (lambda t: t.half()) if half else (lambda t: t)
    all_ctx = torch.cat([o["c1"], o["c2"]], dim=0)
    neg_ctx = torch.cat([o["neg_1"].unsqueeze(1), o["neg_2"].unsqueeze(1)], dim=1)
    s1 = torch.mm(c(o["q"]), c(all_ctx).t())
    n1 = torch.bmm(c(o["q"]).unsqueeze(1), c(neg_ctx).transpose(1, 2)).squeeze(1)
    s2 = torch.mm(c(o["q_sp1"]), c(all_ctx).t())
    n2 = torch.bmm(c(o["q_sp1"]).unsqueeze(1), c(neg_ctx).transpose(1, 2)).squeeze(1)
    B = o["q"].size(0)
    mask = torch.cat([torch.zeros(B, B), torch.eye(B)], dim=1).to(o["q"].device)
    s1 = s1.float().masked_fill(mask.bool(), float("-inf")).type_as(s1)
    s1, s2 = torch.cat([s1, n1], dim=1), torch.cat([s2, n2], dim=1)
    t = torch.arange(B, device=o["q"].device)
    r1 = s1.argsort(dim=1, descending=True).argsort(dim=1)[t, t]
    r2 = s2.argsort(dim=1, descending=True).argsort(dim=1)[t, t + B]
    return r1, r2


def one(B, runs):
    sys.path.insert(0, ROOT)
    import torch
    from multihop_dense_retrieval_amd import criterions, retriever
    torch.cuda.set_device(0)
    m = retriever.RobertaRetriever.random_init("cuda:0", seed=0)
    g = torch.Generator().manual_seed(B)

    def rows(lo, hi):
        lens = torch.randint(lo, hi + 1, (B,), generator=g)
        L = int(lens.max())
        mask = (torch.arange(L)[None, :] < lens[:, None]).long()
        ids = torch.randint(4, 50000, (B, L), generator=g) * mask
        return ids.cuda(), mask.cuda()

    batch = {}
    for key, (lo, hi) in (("q", (20, 30)), ("q_sp", (150, 250)), ("c1", (100, 300)), ("c2", (100, 300)), ("neg1", (100, 300)), ("neg2", (100, 300))):
        batch[f"{key}_input_ids"], batch[f"{key}_mask"] = rows(lo, hi)
    tokens = sum(int(batch[f"{k}_mask"].sum()) for k in ("q", "q_sp", "c1", "c2", "neg1", "neg2"))
    out = {"B": B, "tokens": tokens, "forwards_ms": timed(lambda: m(batch), max(3, runs // 5), warm=2)}
    o = {k: torch.randn(B, 768, device="cuda", generator=torch.Generator(device="cuda").manual_seed(i)) for i, k in
         enumerate(("q", "q_sp1", "c1", "c2", "neg_1", "neg_2"))}
    for mode, name in ((0, "rank_f32_ms"), (1, "rank_o1_ms")):
        out[name] = timed(lambda: criterions.inbatch_rank(o["q"], o["q_sp1"], o["c1"], o["c2"], o["neg_1"], o["neg_2"], mode), runs)
    ctx = torch.cat([o["c1"], o["c2"]]).contiguous()
    neg = torch.stack([o["neg_1"], o["neg_2"]], dim=1).contiguous()
    L = criterions.lib()
    import ctypes
    from multihop_dense_retrieval_amd import _lib
    r1, r2 = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for mode, name in ((0, "kernel_f32_ms"), (1, "kernel_o1_ms")):  # the C entry alone, without the cat / stack / allocations of the Python wrapper
        out[name] = timed(lambda: _lib.check(L.mdr_inbatch_rank(p(o["q"]), p(o["q_sp1"]), p(ctx), p(neg), B, 768, mode, p(r1), p(r2), None, None, None, None,
                                                               None, 0, _lib.current_stream_ptr())), runs)
    out["torch_f32_ms"] = timed(lambda: torch_composition(o, False), runs)
    out["torch_f16_ms"] = timed(lambda: torch_composition(o, True), runs)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="150,1000,3000")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.runs)
    rows = []
    for B in [int(x) for x in a.batches.split(",")]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(B), "--runs", str(a.runs)], timeout=a.timeout, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            sys.exit(f"B = {B} failed with exit status {r.returncode}: stopping")
        rows.append(json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1]))
    cols = ("B", "tokens", "forwards_ms", "rank_f32_ms", "rank_o1_ms", "kernel_f32_ms", "kernel_o1_ms", "torch_f32_ms", "torch_f16_ms")
    table = ["| " + " | ".join(cols) + " | rank_o1 / forwards |", "|" + "---|" * (len(cols) + 1)]
    for r in rows:
        table.append("| " + " | ".join(f"{r[c]:.3f}" if isinstance(r[c], float) else str(r[c]) for c in cols) + f" | {r['rank_o1_ms'] / r['forwards_ms']:.4%} |")
    print("\n".join(table))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
