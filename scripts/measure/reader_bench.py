"""Answer-reader throughput at ELECTRA-large geometry (24 layers, hidden 1024, 16 heads, FFN 4096) with random weights.

    python scripts/measure/reader_bench.py [--configs 32x384,64x384,128x384,32x512,64x512,128x512] [--steps 10] [--warmup 3]

Each (B, L) runs in a child process of its own under a time limit (--timeout seconds); the first child that fails ends the run. A
child times QAModel.decode() -- the forward over every token plus the heads and the span search, what the CLI runs per batch --
on full-length rows (every token real), and prints one JSON line: sequences/s and achieved TFLOP/s, counting
2 x (4 H^2 + 2 H F) + 4 L H FLOP per token and layer (the GEMMs and the two attention matmuls; the heads are < 0.1 %).
"""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flop_per_token(L, H=1024, F=4096, layers=24):
    return layers * (2 * (4 * H * H + 2 * H * F) + 4 * L * H)


def one(B, L, steps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    import transformers
    from multihop_dense_retrieval_amd import reader
    cfg = transformers.ElectraConfig(vocab_size=30522, hidden_size=1024, embedding_size=1024, num_hidden_layers=24, num_attention_heads=16,
                                     intermediate_size=4096, max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12)
    m = reader.QAModel(cfg, types.SimpleNamespace(model_name="google/electra-large-discriminator", sp_pred=True))
    g = torch.Generator(device="cuda").manual_seed(0)
    sd = {}
    for k, shp in m.state_dict().items():
        if k.endswith("LayerNorm.weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(shp, generator=g, device="cuda")
        elif k.endswith("bias") or "embeddings" in k:
            sd[k] = 0.1 * torch.randn(shp, generator=g, device="cuda")
        else:
            sd[k] = (1.0 / shp[1] ** 0.5) * torch.randn(shp, generator=g, device="cuda")
    m.load_state_dict(sd)
    m.to("cuda")
    q = 30
    batch = {"input_ids": torch.randint(1000, 30000, (B, L), device="cuda"), "attention_mask": torch.ones((B, L), dtype=torch.int64, device="cuda"),
             "token_type_ids": torch.zeros((B, L), dtype=torch.int64, device="cuda"), "paragraph_mask": torch.zeros((B, L), dtype=torch.int64, device="cuda"),
             "sent_offsets": torch.arange(q + 2, q + 2 + 40 * 8, 8, device="cuda").repeat(B, 1)}
    batch["token_type_ids"][:, q + 2:] = 1
    batch["paragraph_mask"][:, q + 2:L - 1] = 1
    for _ in range(warmup):
        m.decode(batch, 30)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        res = m.decode(batch, 30)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    assert torch.isfinite(res["span_score"].float()).all()
    seqs = B / (ms / 1e3)
    tflops = flop_per_token(L) * B * L / (ms / 1e3) / 1e12
    est = 0.7e15 / flop_per_token(L) / L  # the issue's estimate: ~0.7 PFLOP/s effective
    print(json.dumps({"B": B, "L": L, "ms_per_batch": round(ms, 3), "seq_per_s": round(seqs, 1), "tflops": round(tflops, 1),
                      "gflop_per_token": round(flop_per_token(L) / 1e9, 3), "estimate_seq_per_s": round(est, 1), "steps": steps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="32x384,64x384,128x384,32x512,64x512,128x512")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--one", default=None, help="BxL: run one configuration in this process")
    a = ap.parse_args()
    if a.one:
        B, L = map(int, a.one.split("x"))
        one(B, L, a.steps, a.warmup)
        return
    for c in a.configs.split(","):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", c, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                           timeout=a.timeout)
        if r.returncode != 0:
            print(f"reader_bench: {c} exited with {r.returncode}; stopping", file=sys.stderr)
            sys.exit(1)


if __name__ == "__main__":
    main()
