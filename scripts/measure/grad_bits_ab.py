"""SHA-256 of every output of every training brick under a given build of the library, to hold two builds of the same sources bit for bit:

    python scripts/measure/grad_bits_ab.py PATH/TO/libmdrhip_variant.so [--out digests.json]

Run it once per library and compare the two files (`cmp a.json b.json`): a refactor of the bricks' plumbing must leave them equal. The parent
sets MDR_LIB_PATH for a fresh child process under a time limit; the child runs each brick's low-level function on inputs drawn from a fixed CPU
seed and prints {case: digest} as one JSON line. Nothing is compared with a reference here: the bricks' own GPU tests do that.

LayerNorm (layer_norm_backward) and embedding (embedding_plan, embedding_backward, embedding_scatter): M or cap in 4, 8, 64, 68, 132 at H = 64
and 768, which is S = 1 (no reduce for the LayerNorm), 2, 16 (every strand of the reduce holds one chunk), 17 (strand 0 wraps) and 33 chunks of 4
rows -- asserted through backward_chunks --, accumulate 0 and 1, all rows valid and one short; the LayerNorm with x in fp16 and in fp32; the
embedding with a 50-row word table and a 40-row position table, so ids repeat. gather_cls_backward on the same H. attention_backward: modes 0
and 3, 1 and 12 heads, sequences of 1, 17, 64 and 65 tokens, max_len 128. linear_backward, one FusedAdam.step, one momentum_update and the
in-batch loss forward and backward: one small case each (only their host prologue is shared code).
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SEED = 20250
CHILD_LIMIT_S = 120
ROWS_TO_CHUNKS = {4: 1, 8: 2, 64: 16, 68: 17, 132: 33}
HS = (64, 768)
VOCAB, MAX_POS, PAD = 50, 40, 1
ATTN_LENS, ATTN_MAX_LEN = (1, 17, 64, 65), 128


def child():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from multihop_dense_retrieval_amd import attention, criterions, embedding, layernorm, linear, optim
    out = {}

    def rng(*key):
        return np.random.default_rng([SEED, *key])

    def cuda(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def normal(r, shape, dtype, scale=1.0):
        return cuda((scale * r.standard_normal(shape)).astype(dtype))

    def put(case, names, tensors):
        for name, t in zip(names, tensors):
            if t is not None:
                out[f"{case} {name}"] = hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()

    scalar = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")  # noqa: E731

    for H in HS:
        for M, S in ROWS_TO_CHUNKS.items():
            assert layernorm.backward_chunks(M, H) == (S, 4) and embedding.backward_chunks(M, H) == (S, 4), (M, H)
            for accumulate in (0, 1):
                for valid in (M, M - 1):
                    for x16 in (False, True):  # the trunk's operand combinations: fp32 in + fp16 residual + fp16 dy2, fp16 in + fp32 residual + fp32 dy2
                        r = rng(1, H, M, accumulate, valid, int(x16))
                        x = normal(r, (M, H), np.float16 if x16 else np.float32)
                        res = normal(r, (M, H), np.float32 if x16 else np.float16)
                        dy16, dy2 = normal(r, (M, H), np.float16), normal(r, (M, H), np.float32 if x16 else np.float16)
                        g, dg, db = normal(r, H, np.float32), normal(r, H, np.float32), normal(r, H, np.float32)
                        got = layernorm.layer_norm_backward(x, res, dy16, dy2, g, 1e-5, None if valid == M else scalar(valid), True, True, dg, db, bool(accumulate))
                        put(f"layernorm H={H} M={M} acc={accumulate} rows={valid} x16={int(x16)}", ("dx16", "dx32", "dg", "db"), got)
                    # the embedding: cap = M tokens of two sequences, ids drawn from 50 rows (they repeat), positions 2, 3, ... as RoBERTa counts them
                    r = rng(2, H, M, accumulate, valid)
                    ids = cuda(r.integers(0, VOCAB, (2, M)).astype(np.int64))
                    half = M // 2
                    src = np.concatenate([np.arange(half), M + np.arange(M - half)]).astype(np.int32)
                    pid = np.concatenate([np.arange(half), np.arange(M - half)]).astype(np.int32) + 1 + PAD
                    tok_src, tok_pid, total = cuda(src), cuda(pid), scalar(valid)
                    word, pos = normal(r, (VOCAB, H), np.float32, 0.1), normal(r, (MAX_POS, H), np.float32, 0.1)
                    type0, g = normal(r, H, np.float32, 0.1), normal(r, H, np.float32)
                    dy16, dy2 = normal(r, (M, H), np.float16), normal(r, (M, H), np.float32)
                    olds = [normal(r, s, np.float32) for s in ((VOCAB, H), (MAX_POS, H), H, H, H)]
                    case = f"embedding H={H} cap={M} acc={accumulate} total={valid}"
                    plan = embedding.embedding_plan(ids, tok_src, tok_pid, total, M, VOCAB, MAX_POS, PAD)
                    d32 = torch.zeros((M, H), dtype=torch.float32, device="cuda")
                    got = embedding.embedding_backward(ids, tok_src, tok_pid, total, M, word, pos, type0, g, 1e-5, dy16, dy2, plan, *[t.clone() for t in olds], d32,
                                                       bool(accumulate))
                    put(case + " backward", ("dword", "dpos", "dtype0", "dg", "db", "d32"), got)
                    got = embedding.embedding_scatter(d32, plan, VOCAB, MAX_POS, *[t.clone() for t in olds[:3]], bool(accumulate))
                    put(case + " scatter", ("dword", "dpos", "dtype0"), got)
                    lay = embedding.plan_layout(M)  # the sections the plan defines: the header, both orders and keys up to total
                    put(case + " plan", ("header", "word order", "pos order", "word keys", "pos keys"),
                        [plan[:8]] + [plan[lay[t][k]: lay[t][k] + valid] for k in ("order", "key") for t in ("word", "pos")])
        r = rng(3, H)
        cu = cuda(np.array([0, 3, 3, 9], dtype=np.int32))
        put(f"gather_cls H={H}", ("acc",), [layernorm.gather_cls_backward(normal(r, (3, H), np.float16), cu, normal(r, (9, H), np.float16))])

    cu_h = np.concatenate([[0], np.cumsum(ATTN_LENS)]).astype(np.int32)
    for heads in (1, 12):
        for mode in (attention.MODE_ALL, attention.MODE_CLS):
            r = rng(4, heads, mode)
            T, hidden = int(cu_h[-1]), 64 * heads
            qkv = normal(r, (T, 3 * hidden), np.float16)
            dctx = normal(r, (len(ATTN_LENS) if mode == attention.MODE_CLS else T, hidden), np.float16)
            put(f"attention heads={heads} mode={mode}", ("dqkv",), [attention.attention_backward(qkv, dctx, cuda(cu_h), heads, ATTN_MAX_LEN, mode)])

    for M, N, K in ((1, 64, 64), (65, 192, 64)):
        r = rng(5, M, N, K)
        x, w, dy, pre = normal(r, (M, K), np.float16), normal(r, (N, K), np.float16, 0.1), normal(r, (M, N), np.float16), normal(r, (M, N), np.float16)
        got = linear.linear_backward(x, w, dy, pre, None, True, normal(r, (N, K), np.float32), normal(r, N, np.float32), True)
        put(f"linear M={M} N={N} K={K}", ("dx", "dw", "db"), got)

    r = rng(6)
    shapes = ((1,), (65,), (64, 64), (4097,))
    params = [torch.nn.Parameter(normal(r, s, np.float32)) for s in shapes]
    opt = optim.FusedAdam(params, lr=1e-3, weight_decay=0.01, fp16_copies=True)
    for p in params:
        p.grad = normal(r, tuple(p.shape), np.float32, 65536.0)
    opt.step()
    for i, p in enumerate(params):
        put(f"optim tensor {i}", ("p", "grad", "exp_avg", "exp_avg_sq", "half"),
            (p, p.grad, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], opt.half(p) if p.dim() >= 2 else None))
    put("optim", ("state",), [opt._state[:12]])
    ks, qs = [normal(r, s, np.float32) for s in shapes], [normal(r, s, np.float32) for s in shapes]
    optim.momentum_update(ks, qs, 0.999)
    put("momentum_update", [f"k{i}" for i in range(len(ks))], ks)

    B, d, K = 5, 64, 3
    for fp16 in (False, True):
        r = rng(7, int(fp16))
        leaves = {k: normal(r, (B, d), np.float32).requires_grad_(True) for k in ("q", "q_sp1", "c1", "c2", "neg_1", "neg_2")}
        loss = criterions.mhop_loss_outputs(leaves, argparse.Namespace(fp16=fp16), queue=normal(r, (K, d), np.float32))
        loss.backward()
        put(f"inbatch fp16={int(fp16)}", ["loss"] + [f"d{k}" for k in leaves], [loss] + [t.grad for t in leaves.values()])

    torch.cuda.synchronize()
    print(json.dumps(out, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?", help="the library to load (MDR_LIB_PATH of the child)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    if not a.lib or not os.path.exists(a.lib):
        sys.exit(f"no such library: {a.lib}")
    env = dict(os.environ, MDR_LIB_PATH=os.path.abspath(a.lib))
    p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env)
    if p.returncode != 0:
        print(f"{a.lib}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
        sys.exit(1)
    digests = json.loads(p.stdout.strip().split("\n")[-1])
    text = json.dumps(digests, indent=0, sort_keys=True) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(f"{len(digests)} digests, sha256 of all: {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main()
