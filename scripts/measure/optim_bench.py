"""Time the optimizer step (optim.FusedAdam: mdr_optim_step of include/mdr_optim.h) and the momentum encoder's EMA (optim.momentum_update)
against torch's composition of the same work on the same device, on the parameter list of RoBERTa-base:

    python scripts/measure/optim_bench.py [--out profiles/optim_bench.md] [--iters 30] [--reps 5] [--plain-lib PATH]

The parameters are retriever.expected_state_dict_shapes(RobertaConfig()) (about 125 M elements in about 200 tensors); the pooler's two
tensors get no gradient, as in every training step of the retriever. Both sides keep fp16 copies of the Linear weights (every two-dimensional
parameter outside the embeddings that has a gradient) and zero the gradients.
  ours:   FusedAdam.step(): three kernels, no synchronisation.
  torch:  clip_grad_norm_(params, 2.0), torch.optim.Adam(fused=True).step(), zero_grad(set_to_none=False), and w.half() of the Linear
          weights. It has no loss scale to undo and no overflow check: apex's would add a pass and a host synchronisation.
  EMA:    momentum_update over the whole list against the reference's loop (param_k.data = param_k.data * m + param_q.data * (1. - m)) and
          against torch._foreach_mul_ / _foreach_add_.
One timed step is `--reps` calls between two device events, divided by `--reps`; the figure is the median of `--iters` steps after 3 warm-up
steps. Bytes: what the step must move -- g read twice (the norm, the update) and written once (the zeroing), p, m, v read and written once,
the fp16 copies written once; TB/s = bytes / time, beside the 6.29 TB/s a float4 copy reaches on this device. The kernels apart from the
profiler's kernel times. --plain-lib: a build of the same sources with -DMDR_OPTIM_NT=0 (plain loads and stores in the sweeps, where the
product build has nontemporal ones), measured in a child process of its own through MDR_LIB_PATH. The trajectory errors of tests/test_optim_gpu.py (20 steps, 12 tensors) are measured
here too. Every leg runs in a child process under a time limit; the first failure stops the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CHILD_LIMIT_S = 240
COPY_TBS = 6.29
KERNELS = {"norm_kernel_ms": "optim_norm_kernel", "finalize_kernel_ms": "optim_finalize_kernel", "update_kernel_ms": "optim_update_kernel"}


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


def make_params(torch, retriever, seed):
    shapes = retriever.expected_state_dict_shapes(retriever.RobertaConfig())
    g = torch.Generator(device="cuda").manual_seed(seed)
    return {k: torch.nn.Parameter(0.02 * torch.randn(s, generator=g, device="cuda")) for k, s in shapes.items()}


def groups_of(params):
    no_decay = ["bias", "LayerNorm.weight"]
    return [{"params": [p for n, p in params.items() if not any(nd in n for nd in no_decay)], "weight_decay": 0.01},
            {"params": [p for n, p in params.items() if any(nd in n for nd in no_decay)], "weight_decay": 0.0}]


def child(iters, reps):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from multihop_dense_retrieval_amd import optim, retriever
    r = {}
    params = make_params(torch, retriever, 1)
    live = {n: p for n, p in params.items() if "pooler" not in n}
    linear = [p for n, p in live.items() if p.dim() == 2 and "embeddings" not in n]
    n_live, n_lin = sum(p.numel() for p in live.values()), sum(p.numel() for p in linear)
    r.update(tensors=len(params), elements=sum(p.numel() for p in params.values()), live_elements=n_live, linear_elements=n_lin)
    r["step_bytes"] = n_live * 36 + n_lin * 2
    gen = torch.Generator(device="cuda").manual_seed(2)
    for p in live.values():
        p.grad = 2.0 ** 16 * 1e-3 * torch.randn(p.shape, generator=gen, device="cuda")
    opt = optim.FusedAdam(groups_of(params), lr=2e-5, eps=1e-8, max_grad_norm=2.0, fp16_copies=linear)
    opt.step()
    r["chunks"] = opt._n_chunks
    r["fused_step_ms"] = median_ms(opt.step, iters, reps)
    st = opt.read_state()
    r["adam_steps"], r["skipped"] = st["adam_step"], st["skipped_total"]
    from torch.profiler import ProfilerActivity, profile
    try:  # the kernels apart, from the device's own kernel times
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                opt.step()
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            for key, pat in KERNELS.items():
                if pat in ev.key:
                    r[key] = r.get(key, 0.0) + ev.device_time_total / iters / 1000.0
    except Exception as e:  # the split is an extra: without a working profiler the table shows "-" there, the totals stand
        r["profiler_error"] = repr(e)[:200]
    # the EMA against the reference's loop, on a second copy of the list
    params_k = make_params(torch, retriever, 3)
    ks, qs = list(params_k.values()), list(params.values())
    m = 0.999
    r["ema_bytes"] = r["elements"] * 12
    r["ema_ms"] = median_ms(lambda: optim.momentum_update(ks, qs, m), iters, reps)

    def reference_loop():
        for pk, pq in zip(ks, qs):
            pk.data = pk.data * m + pq.data * (1. - m)

    def foreach():
        kd = [p.data for p in ks]
        torch._foreach_mul_(kd, m)
        torch._foreach_add_(kd, [p.data for p in qs], alpha=1. - m)

    r["ema_torch_loop_ms"] = median_ms(reference_loop, iters, reps)
    r["ema_torch_foreach_ms"] = median_ms(foreach, iters, reps)
    del opt, params_k, ks, qs
    # torch's composition on the same parameters
    if os.environ.get("MDR_OPTIM_BENCH_OURS_ONLY") != "1":
        for p in live.values():
            p.grad = 1e-3 * torch.randn(p.shape, generator=gen, device="cuda")
        topt = torch.optim.Adam(groups_of(params), lr=2e-5, eps=1e-8, fused=True)
        everything = list(params.values())
        halves = []

        def theirs():
            torch.nn.utils.clip_grad_norm_(everything, 2.0)
            topt.step()
            topt.zero_grad(set_to_none=False)
            halves[:] = [w.detach().half() for w in linear]

        r["torch_step_ms"] = median_ms(theirs, iters, reps)

        def theirs_adam_only():
            topt.step()

        r["torch_adam_only_ms"] = median_ms(theirs_adam_only, iters, reps)
        # the trajectory of tests/test_optim_gpu.py
        import optim_ref as ref
        start, targets = ref.trajectory_start()
        want = ref.torch_trajectory(start, targets, 20, torch.float64)
        r["e_torch"] = max(ref.traj_errors(ref.torch_trajectory(start, targets, 20, torch.float32, "cuda"), want))
        ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).cuda()) for p in start]
        ts = [torch.from_numpy(t).cuda() for t in targets]
        fopt = optim.FusedAdam([{"params": ps[0::2], "weight_decay": ref.TRAJ["weight_decay"]}, {"params": ps[1::2], "weight_decay": 0.0}],
                               lr=ref.TRAJ["lr"], betas=ref.TRAJ["betas"], eps=ref.TRAJ["eps"], max_grad_norm=ref.TRAJ["max_grad_norm"])
        for _ in range(20):
            for p, t in zip(ps, ts):
                g = 2.0 ** 16 * (p.detach() - t)
                if p.grad is None:
                    p.grad = g
                else:
                    p.grad.copy_(g)
            fopt.step()
        r["e_ours"] = max(ref.traj_errors([p.detach().cpu().numpy() for p in ps], want))
    print(json.dumps(r))


def run_child(a, env_extra):
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--reps", str(a.reps), "--child"]
    p = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env_extra))
    if p.returncode != 0:
        print(f"child {env_extra}: exit {p.returncode}\n{p.stderr[-3000:]}", flush=True)
        sys.exit(1)  # the first failure stops the run: nothing more is started on the device
    r = json.loads(p.stdout.strip().split("\n")[-1])
    print(r, flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.md"))
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-lib", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.iters, a.reps)
    r = run_child(a, {})
    nt = run_child(a, {"MDR_LIB_PATH": os.path.abspath(a.plain_lib), "MDR_OPTIM_BENCH_OURS_ONLY": "1"}) if a.plain_lib else None
    f3 = lambda d, k: "-" if d is None or d.get(k) is None else f"{d[k]:.3f}"  # noqa: E731
    tbs = lambda d, k, b: "-" if d is None or d.get(k) is None else f"{d[b] / (d[k] * 1e-3) / 1e12:.2f}"  # noqa: E731
    lines = ["# The optimizer step: optim.FusedAdam (mdr_optim_step) against torch's composition, and the EMA", "",
             "Command: `python scripts/measure/optim_bench.py --iters %d --reps %d%s` (one timed step is %d calls between two device events, divided by "
             "%d; median of %d steps after 3 warm-up steps; one MI355X). RoBERTa-base: %d tensors, %d elements, %d of them with a gradient (the pooler "
             "has none), %d in Linear weights that keep an fp16 copy; %d chunks of 4096. MB: g read twice and zeroed, p, m, v read and written, the "
             "fp16 copies written (36 B per element with a gradient + 2 B per copied one); TB/s = MB / time, beside the %.2f TB/s a float4 copy "
             "reaches on this device. torch: clip_grad_norm_ + Adam(fused=True).step() + zero_grad(set_to_none=False) + .half() of the same Linear "
             "weights; it undoes no loss scale and checks no overflow." % (a.iters, a.reps, " --plain-lib <-DMDR_OPTIM_NT=0 build>" if nt else "", a.reps, a.reps,
                                                                             a.iters, r["tensors"], r["elements"], r["live_elements"],
                                                                             r["linear_elements"], r["chunks"], COPY_TBS), "",
             "| step | MB | ms | TB/s | share of the copy rate | norm kernel ms | finalize kernel ms | update kernel ms |", "|---|---|---|---|---|---|---|---|"]
    for label, d in (("FusedAdam.step() (nontemporal loads and stores: the product build)", r), ("FusedAdam.step(), plain loads and stores (-DMDR_OPTIM_NT=0)", nt)):
        if d is not None:
            share = d["step_bytes"] / (d["fused_step_ms"] * 1e-3) / 1e12 / COPY_TBS
            lines.append(f"| {label} | {d['step_bytes'] / 1e6:.0f} | {f3(d, 'fused_step_ms')} | {tbs(d, 'fused_step_ms', 'step_bytes')} | {share:.0%} | "
                         f"{f3(d, 'norm_kernel_ms')} | {f3(d, 'finalize_kernel_ms')} | {f3(d, 'update_kernel_ms')} |")
    lines.append(f"| torch: clip_grad_norm_ + Adam(fused=True) + zero_grad + .half() | - | {f3(r, 'torch_step_ms')} | - | - | - | - | - |")
    lines.append(f"| torch: Adam(fused=True).step() alone | - | {f3(r, 'torch_adam_only_ms')} | - | - | - | - | - |")
    lines += ["", "| EMA over the whole list | MB | ms | TB/s |", "|---|---|---|---|"]
    for label, d, k in (("momentum_update (mdr_optim_ema)", r, "ema_ms"), ("momentum_update, plain loads and stores", nt, "ema_ms"),
                        ("torch: the reference's loop", r, "ema_torch_loop_ms"), ("torch: _foreach_mul_ + _foreach_add_", r, "ema_torch_foreach_ms")):
        if d is not None:
            lines.append(f"| {label} | {d['ema_bytes'] / 1e6:.0f} | {f3(d, k)} | {tbs(d, k, 'ema_bytes')} |")
    lines += ["", "Trajectory (tests/test_optim_gpu.py: 20 steps of g = S (p - target) on 12 tensors, e the largest |p - p64| / (|p64| + 1e-3)): "
              f"e(FusedAdam) = {r['e_ours']:.3g}, e(torch fp32 Adam + clip_grad_norm_ on the device) = {r['e_torch']:.3g}; the bar is e(ours) <= 2 e(torch)."]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
