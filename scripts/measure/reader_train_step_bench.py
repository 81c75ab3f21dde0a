"""Measure the reader's training step (multihop_dense_retrieval_amd/reader_train.py) at ELECTRA-large geometry (24 x 1024, 16 heads, FFN 4096,
L = 512) on one device:

    python scripts/measure/reader_train_step_bench.py [--batches 64,32] [--steps 3] [--out FILE.json]

Per batch size of the list that fits (a size whose step runs out of memory is reported as such and skipped): the time of a step split into
forward, backward and optimizer (events on the current stream, the median of --steps steps after one warm-up step), and the peak allocated
memory. Then, alone: the reader's embedding backward and its plan at 96 x 512 tokens (H = 1024), and the optimizer step in AdamW mode
against mode 0 on the model's own table, with torch.optim.AdamW over the same tensors as a timing yardstick. Prints one JSON object;
profiles/reader_train_step.md holds a run."""
import argparse
import json
import statistics
import sys
import os
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from multihop_dense_retrieval_amd import embedding, optim, reader_train  # noqa: E402

L = 512


def large_config():
    return types.SimpleNamespace(vocab_size=30522, hidden_size=1024, embedding_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                                 max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu", pad_token_id=0,
                                 hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)


def make_batch(B, seed, sp=True):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(L // 2, L + 1, (B,), generator=g)
    lens[0] = L
    pos = torch.arange(L)[None]
    mask = (pos < lens[:, None]).long()
    ids = torch.randint(1, 30522, (B, L), generator=g) * mask
    tt = ((pos >= 20) & (pos < lens[:, None])).long()
    pm = ((pos >= 22) & (pos < lens[:, None] - 1)).long()
    starts = torch.randint(22, L // 2 - 8, (B, 2), generator=g)
    ends = starts + torch.randint(0, 6, (B, 2), generator=g)
    starts[1::2, 1], ends[1::2, 1] = -1, -1
    so = torch.sort(torch.randint(22, L // 2 - 1, (B, 8), generator=g), 1).values
    batch = {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt, "paragraph_mask": pm, "label": (torch.arange(B) % 4 == 0).long()[:, None],
             "starts": starts, "ends": ends, "sent_offsets": so, "sent_labels": (torch.rand(B, 8, generator=g) < 0.3).long()}
    return {k: v.cuda() for k, v in batch.items()}, int(lens.sum())


def timed(fn, reps):
    """median ms of fn() over reps runs (events on the current stream), after one untimed run"""
    fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def step_split(model, opt, args, batch, steps):
    rows = []
    for s in range(steps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        loss = model(batch, seed=s, half=opt.half)
        ev[1].record()
        opt.scale_loss(loss).backward()
        ev[2].record()
        opt.step()
        ev[3].record()
        torch.cuda.synchronize()
        if s:  # the first step warms up (allocator, table upload)
            rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)])
    med = [statistics.median(r[i] for r in rows) for i in range(3)]
    return {"forward_ms": med[0], "backward_ms": med[1], "optimizer_ms": med[2], "step_ms": sum(med), "loss": float(loss), "state": opt.read_state()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,32")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.manual_seed(0)
    cfg = large_config()
    args = types.SimpleNamespace(model_name="google/electra-large-discriminator", sp_pred=True, sp_weight=0.025, learning_rate=5e-5, adam_epsilon=1e-8,
                                 max_grad_norm=2.0, weight_decay=0.01, gradient_accumulation_steps=1, use_adam=False)
    model = reader_train.TrainableReader(cfg, args).cuda().train()
    opt = reader_train.optimizer_for(model, args)
    res = {"device": torch.cuda.get_device_name(0), "parameters": sum(p.numel() for p in model.parameters()), "L": L, "steps": a.steps, "by_batch": {}}
    for B in [int(x) for x in a.batches.split(",")]:
        batch, tokens = make_batch(B, B)
        torch.cuda.reset_peak_memory_stats()
        try:
            r = step_split(model, opt, args, batch, a.steps)
        except torch.OutOfMemoryError as e:
            res["by_batch"][B] = {"out_of_memory": str(e)[:120]}
            for p in model.parameters():
                p.grad = None
            torch.cuda.empty_cache()
            continue
        r.update(tokens=tokens, peak_allocated_gib=torch.cuda.max_memory_allocated() / 2 ** 30)
        res["by_batch"][B] = r
        print(f"# B={B}", json.dumps(r), flush=True)
    # ---- the optimizer alone on the model's table: AdamW against mode 0, and torch's AdamW over the same tensors
    for p in model.parameters():
        p.grad = torch.randn_like(p) * 65536.0
    o = {}
    for name, decoupled in (("adamw_ms", True), ("mode0_ms", False)):
        opt.decoupled_weight_decay = decoupled
        o[name] = timed(lambda: opt.step(), 5)  # (zero_grads leaves g = 0 behind: the update still moves the same bytes)
    opt.decoupled_weight_decay = True
    topt = torch.optim.AdamW([{"params": [p for p in model.parameters() if p.dim() > 1], "weight_decay": 0.01},
                              {"params": [p for p in model.parameters() if p.dim() == 1], "weight_decay": 0.0}], lr=5e-5, eps=1e-8)
    o["torch_adamw_ms"] = timed(lambda: topt.step(), 3)
    o["torch_adamw_with_clip_ms"] = timed(lambda: (torch.nn.utils.clip_grad_norm_(model.parameters(), 2.0), topt.step()), 3)
    res["optimizer_alone"] = o
    del topt
    for p in model.parameters():
        p.grad = None
    torch.cuda.empty_cache()
    # ---- the embedding backward and its plan alone at 96 x 512 tokens
    B = 96
    batch, tokens = make_batch(B, 7)
    P = dict(model.named_parameters())
    E = "encoder.embeddings."
    cap = B * L
    src = torch.nonzero(batch["attention_mask"].reshape(-1)).reshape(-1).to(torch.int32)
    total = torch.tensor([src.numel()], dtype=torch.int32, device="cuda")
    src = torch.cat([src, torch.zeros(cap - src.numel(), dtype=torch.int32, device="cuda")])
    dy = torch.randn(cap, 1024, device="cuda").half()
    tab = [P[E + n].detach() for n in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight")]
    plan = embedding.reader_embedding_plan(batch["input_ids"], src, total, cap, L, 30522, 512, 0)
    outs = [torch.zeros_like(t) for t in tab] + [torch.zeros(1024, device="cuda")]
    e = {"tokens": tokens, "cap": cap}
    e["plan_ms"] = timed(lambda: embedding.reader_embedding_plan(batch["input_ids"], src, total, cap, L, 30522, 512, 0), 5)
    e["backward_ms"] = timed(lambda: embedding.reader_embedding_backward(batch["input_ids"], batch["token_type_ids"], src, total, cap, L, *tab, 1e-12, dy, None, plan,
                                                                         *outs, accumulate=True), 5)
    e["backward_overwrite_ms"] = timed(lambda: embedding.reader_embedding_backward(batch["input_ids"], batch["token_type_ids"], src, total, cap, L, *tab, 1e-12, dy, None,
                                                                                   plan, *outs, accumulate=False), 5)
    res["embedding_backward_96x512"] = e
    text = json.dumps(res)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
