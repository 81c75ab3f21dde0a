"""Time the reader's training loss and heads (include/mdr_reader_loss.h), forward and backward, against torch's own composition of the same
operations on the same device:

    python scripts/measure/reader_loss_bench.py [--out TABLE.md] [--iters 30]

Shapes: B = 64 and 96 rows of L = 512, H = 1024 (ELECTRA-large, the shipping rows of the reader), lengths uniform in [L / 2, L], A = 8 candidate
spans, NS = 30 sentence markers, the paragraph mask from position 20 to the row's end. Legs of one shape run in ONE child process, interleaved
round by round: heads forward, loss forward, loss backward, heads backward (each one C call on the packed rows), and torch: fp16 F.linear heads on
the padded [B, L, H] batch, the reference's loss formula in fp32 (CrossEntropyLoss per candidate, BCEs), backward() to the hidden states and the
head parameters. Times are medians of `--iters` rounds after 3 warm-up rounds, by device events around one call. The heads backward's GB/s
counts the bytes its token pass must move, 2 T H 2 (one read of h16, one write of d_h), over the WHOLE call's time (token pass, the strand
reduce of the dw partial sums, the bias and rank kernels), so the token pass alone is faster than the figure. Every child runs under a time
limit; the first failure stops the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(64, 512), (96, 512)]
H, A, NS, PARA = 1024, 8, 30, 20
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


def child(B, L, iters):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import reader_loss as rl
    F = torch.nn.functional
    rng = np.random.default_rng([B, L])
    lens = rng.integers(L // 2, L + 1, size=B)
    cu_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T = int(cu_h[-1])
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    h16 = cuda(rng.standard_normal((T, H)).astype(np.float16))
    dense16 = cuda(rng.standard_normal((B, H)).astype(np.float16))
    cu = cuda(cu_h)
    pmask = np.zeros((B, L), np.int64)
    starts, ends = np.full((B, A), -1, np.int64), np.full((B, A), -1, np.int64)
    offs = np.zeros((B, NS), np.int64)
    for b, n in enumerate(lens):
        pmask[b, PARA:n - 1] = 1
        k = int(rng.integers(1, A + 1))
        starts[b, :k] = rng.integers(PARA, n - 1, size=k)
        ends[b, :k] = np.minimum(starts[b, :k] + rng.integers(0, 8, size=k), n - 2)
        m = int(rng.integers(NS // 2, NS + 1))
        offs[b, :m] = np.sort(rng.integers(PARA, n, size=m))
    batch = {"paragraph_mask": cuda(pmask), "starts": cuda(starts), "ends": cuda(ends), "label": cuda(rng.integers(0, 2, size=(B, 1))),
             "sent_offsets": cuda(offs), "sent_labels": cuda(rng.integers(0, 2, size=(B, NS)))}
    s = 1.5 / np.sqrt(H)
    P = {"qa_outputs.weight": cuda((s * rng.standard_normal((2, H))).astype(np.float32)), "qa_outputs.bias": cuda(np.zeros(2, np.float32)),
         "rank.weight": cuda((s * rng.standard_normal((1, H))).astype(np.float32)), "rank.bias": cuda(np.zeros(1, np.float32)),
         "sp.weight": cuda((s * rng.standard_normal((1, H))).astype(np.float32)), "sp.bias": cuda(np.zeros(1, np.float32))}
    w16, b32 = rl.head_rows16(P, True, h16.device)
    pm, of = batch["paragraph_mask"], batch["sent_offsets"]
    ints = {k: batch[k] for k in ("starts", "ends", "sent_offsets", "sent_labels")}
    ints["label"] = batch["label"].reshape(-1).contiguous()
    g0 = torch.full((1,), 64.0, device="cuda")
    state = {}

    def heads_fwd():
        state["scores"] = rl.heads_forward(h16, dense16, cu, pm, of, w16, b32, True)

    def loss_fwd():
        st, en, rk, sp = state["scores"]
        state["loss"] = rl._QALoss.apply(st, en, rk, sp, ints, (B, L, A, NS), 1.0)

    def loss_bwd():
        st, en, rk, sp = state["scores"]
        out = [torch.empty_like(t) for t in (st, en, rk, sp)]
        from multihop_dense_retrieval_amd import _lib
        p = _lib.ptr
        _lib.call(rl.lib().mdr_reader_loss_backward, p(st), p(en), p(rk), p(sp), p(ints["starts"]), p(ints["ends"]), p(ints["label"]), p(ints["sent_offsets"]),
                  p(ints["sent_labels"]), B, L, A, NS, 1.0, p(g0), *[p(t) for t in out], dev=h16.device)
        state["grads"] = out

    bufs = {}

    def heads_bwd():
        g = state["grads"]
        bufs["out"] = rl.heads_backward(h16, dense16, cu, pm, of, w16, g[0], g[1], g[2], g[3], bufs.get("out"))

    # torch's composition on the padded batch
    pad = torch.zeros((B, L, H), dtype=torch.float16, device="cuda")
    for b, n in enumerate(lens):
        pad[b, :n] = h16[int(cu_h[b]):int(cu_h[b + 1])]
    pad.requires_grad_(True)
    dense_t = dense16.clone().requires_grad_(True)
    tp = {k: v.half().requires_grad_(True) for k, v in P.items()}
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, reduction="none")

    def torch_step():
        logits = F.linear(pad, tp["qa_outputs.weight"], tp["qa_outputs.bias"])
        st, en = (logits[..., i].float().masked_fill(pm != 1, float("-inf")) for i in (0, 1))
        rk = F.linear(torch.tanh(dense_t), tp["rank.weight"], tp["rank.bias"]).float()
        sp = F.linear(torch.gather(pad, 1, of.unsqueeze(2).expand(-1, -1, H)), tp["sp.weight"], tp["sp.bias"]).squeeze(2).float()
        label = batch["label"]
        sp_loss = ((F.binary_cross_entropy_with_logits(sp, batch["sent_labels"].float(), reduction="none") * of) * label).sum()
        rank_loss = F.binary_cross_entropy_with_logits(rk, label.float(), reduction="sum")
        lt = torch.stack([ce(st, a) for a in torch.unbind(batch["starts"], 1)], 1) + torch.stack([ce(en, a) for a in torch.unbind(batch["ends"], 1)], 1)
        lp = (-lt).masked_fill(-lt == 0, float("-inf"))
        m = torch.exp(lp).sum(1)
        span = -torch.log(torch.where(m != 0, m, torch.ones_like(m))).sum()  # (no host synchronisation: uncounted rows add log 1)
        loss = (rank_loss + span + sp_loss) * 64.0
        torch.autograd.grad(loss, [pad, dense_t] + list(tp.values()))

    legs = {"heads_fwd": heads_fwd, "loss_fwd": loss_fwd, "loss_bwd": loss_bwd, "heads_bwd": heads_bwd, "torch_fwd_bwd": torch_step}
    res = {"B": B, "L": L, "tokens": T}
    res.update(timed(legs, iters))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file (profiles/reader_loss_bench.md holds one with its commentary)")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--child", nargs=2, type=int, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.iters)
    rows = []
    for B, L in SHAPES:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--child", str(B), str(L)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            print(f"{B} x {L}: exit {p.returncode}\n{p.stderr[-3000:]}", flush=True)
            sys.exit(1)  # the first failure stops the run: nothing more is started on the device
        rows.append(json.loads(p.stdout.strip().split("\n")[-1]))
        print(rows[-1], flush=True)
    lines = ["| B | L | tokens | heads fwd ms | loss fwd ms | loss bwd ms | heads bwd ms | all four ms | torch fwd + bwd ms | torch / all four | heads bwd GB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        ours = r["heads_fwd"] + r["loss_fwd"] + r["loss_bwd"] + r["heads_bwd"]
        lines.append(f"| {r['B']} | {r['L']} | {r['tokens']} | {r['heads_fwd']:.3f} | {r['loss_fwd']:.3f} | {r['loss_bwd']:.3f} | {r['heads_bwd']:.3f} | {ours:.3f} | "
                     f"{r['torch_fwd_bwd']:.3f} | {r['torch_fwd_bwd'] / ours:.2f} | {4 * r['tokens'] * H / r['heads_bwd'] / 1e6:.0f} |")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

if __name__ == "__main__":
    main()
