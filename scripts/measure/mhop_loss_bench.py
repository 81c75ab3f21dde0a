"""Time the in-batch loss, forward plus backward (criterions.mhop_loss_outputs: mdr_inbatch_loss_forward / _backward), against the torch-autograd
composition of the reference's formula (mm / bmm / masked_fill / cat / CrossEntropyLoss, fp32, or fp16 matmuls with an fp32 loss for mode O1) on
the same device:

    python scripts/measure/mhop_loss_bench.py [--out profiles/mhop_loss_bench.md] [--iters 20]

Shapes (B, K) = (150, 0), (150, 76800), (3000, 0) at d = 768, both modes. Every configuration runs in a child process of its own under a time limit;
the first failure stops the run. Times are medians of `--iters` steps after 3 warm-up steps, by device events around one step.
"""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = [(150, 0), (150, 76800), (3000, 0)]
D = 768
CHILD_LIMIT_S = 120


def child(B, K, mode, which, iters):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mhop_loss_ref as ref
    from multihop_dense_retrieval_amd import criterions
    inp, queue = ref.make_inputs(B, D, K, seed=1)
    t = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in inp.items()}
    qd = torch.from_numpy(queue).cuda() if K else None
    args = types.SimpleNamespace(fp16=mode == 1)
    eye = torch.cat([torch.zeros(B, B), torch.eye(B)], dim=1).bool().cuda()
    tgt = torch.arange(B, device="cuda")
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1)

    def torch_step():
        c = (lambda x: x.half()) if mode == 1 else (lambda x: x)
        all_ctx = torch.cat([t["c1"], t["c2"]], dim=0)
        neg = torch.cat([t["neg_1"].unsqueeze(1), t["neg_2"].unsqueeze(1)], dim=1)
        loss = 0
        for h, x in enumerate((t["q"], t["q_sp1"])):
            s = torch.mm(c(x), c(all_ctx).t())
            n = torch.bmm(c(x).unsqueeze(1), c(neg).transpose(1, 2)).squeeze(1)
            if h == 0:
                s = s.float().masked_fill(eye, float("-inf")).type_as(s)
            cols = [s, n] + ([torch.mm(c(x), c(qd).t())] if K else [])
            loss = loss + ce(torch.cat(cols, dim=1).float(), tgt + h * B)
        loss.backward()

    def hip_step():
        criterions.mhop_loss_outputs(t, args, queue=qd).backward()

    step = hip_step if which == "hip" else torch_step
    times = []
    for i in range(3 + iters):
        for v in t.values():
            v.grad = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        torch.cuda.synchronize()
        if i >= 3:
            times.append(a.elapsed_time(b))
    times.sort()
    print(json.dumps({"B": B, "K": K, "mode": mode, "which": which, "ms": times[len(times) // 2], "min_ms": times[0]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mhop_loss_bench.md"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--child", nargs=4, default=None)
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), int(a.child[1]), int(a.child[2]), a.child[3], a.iters)
    rows = []
    for B, K in SHAPES:
        for mode in (0, 1):
            r = {}
            for which in ("hip", "torch"):
                cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--child", str(B), str(K), str(mode), which]
                p = subprocess.run(cmd, capture_output=True, text=True)
                if p.returncode != 0:
                    print(f"B={B} K={K} mode={mode} {which}: exit {p.returncode}\n{p.stderr[-2000:]}", flush=True)
                    sys.exit(1)  # the first failure stops the run: nothing more is started on the device
                r[which] = json.loads(p.stdout.strip().split("\n")[-1])
                print(r[which], flush=True)
            rows.append((B, K, mode, r["hip"]["ms"], r["torch"]["ms"]))
    lines = ["# In-batch loss, forward + backward: HIP kernels against the torch-autograd composition", "",
             "Command: `python scripts/measure/mhop_loss_bench.py --iters %d` (d = 768; median of %d steps after 3 warm-up steps, device events; one MI355X)." % (a.iters, a.iters),
             "", "| B | K | mode | HIP ms | torch ms | torch / HIP |", "|---|---|---|---|---|---|"]
    for B, K, mode, hip, tor in rows:
        lines.append(f"| {B} | {K} | {'O1' if mode else 'F32'} | {hip:.3f} | {tor:.3f} | {tor / hip:.2f} |")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
