"""End-to-end QA cost per question on one MI355X, a synthetic lower bound of the CLI's (see below): retrieval (hop-1 encode, search, device hop-2 assembly, hop-2 encode, search, path
ranking), reader input assembly (mdr_reader_assemble), reader forward + heads + span search (QAModel.decode), host decode of the
selected chain (prepare + text decode), for --topk in {1, 2, 5, 10, 20, 50} at --batch-size 1 and 100.

    python scripts/measure/end2end_bench.py [--rows 1000000] [--topks 1,2,5,10,20,50] [--batches 1,100] [--steps 3]

Random weights at roberta-base (retriever) and ELECTRA-large (reader) geometry; a synthetic index of --rows x 768; a synthetic hop-2
token arena (mhop.SyntheticTwoHop) and a synthetic QA arena (passages of 2-5 sentences, 60-250 WordPieces). Device legs are timed
with HIP events, the host decode with a host clock. Also measured on this host's CPU: QAEvalDataset + qa_collate per 2-passage chain
(the host cost the arena removes) and the one-off QA arena build rate with 16 workers, both with the toy WordPiece vocabulary of
tests/golden/reader_electra_tiny on synthetic text. Not timed: the CLI's host work around the device loop -- question tokenisation for the
retriever and the reader (question ids are random on the device here), TwoHopPipeline's plumbing and the host-side rank_paths -- so the
questions/s column is an upper bound of the CLI's throughput (a lower bound of its time). Each configuration runs in a child process under --timeout; one JSON line each.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
VOCAB = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny", "vocab.txt")


def _words(rng, n):
    w = [ln for ln in open(VOCAB).read().split("\n") if ln and not ln.startswith("[") and not ln.startswith("##")]
    return [w[i] for i in rng.integers(0, len(w), n)]


def synthetic_corpus(n, seed=0):
    import numpy as np
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(n):
        ns = int(rng.integers(2, 6))
        total = int(rng.integers(60, 251))
        per = max(1, total // ns)
        out[str(i)] = {"title": f"Title {i}", "text": "", "sents": [" ".join(_words(rng, per)) + " ." for _ in range(ns)]}
    return out


def host_costs(n_chains=200, n_build=20000):
    """QAEvalDataset + qa_collate per chain, and the QA arena build rate with 16 workers (CPU only)."""
    sys.path.insert(0, ROOT)
    import transformers
    from functools import partial
    from multihop_dense_retrieval_amd import qa_arena, qa_data
    tok = transformers.BertTokenizer(VOCAB, do_lower_case=True)
    corpus = synthetic_corpus(max(n_build, 2 * n_chains))
    items = [{"_id": f"q{i}", "question": "which film was released first?", "candidate_chains": [[corpus[str(2 * i)], corpus[str(2 * i + 1)]]]}
             for i in range(n_chains)]
    t0 = time.perf_counter()
    ds = qa_data.QAEvalDataset(tok, items, max_seq_len=512, max_q_len=64)
    samples = [ds[i] for i in range(len(ds))]
    t1 = time.perf_counter()
    partial(qa_data.qa_collate, pad_id=tok.pad_token_id)(samples)
    t2 = time.perf_counter()
    t3 = time.perf_counter()
    qa_arena.QAArena.from_corpus({str(i): corpus[str(i)] for i in range(n_build)}, tok, workers=16)
    t4 = time.perf_counter()
    print(json.dumps({"leg": "host", "prepare_tokenize_ms_per_chain": round((t1 - t0) / n_chains * 1e3, 3),
                      "collate_ms_per_chain": round((t2 - t1) / n_chains * 1e3, 3), "qa_arena_build_passages_per_s_16_workers": round(n_build / (t4 - t3), 1),
                      "n_build": n_build}), flush=True)


def one(rows, B, k, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import transformers
    from multihop_dense_retrieval_amd import end2end, index, mhop, qa_arena, reader
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cuda").manual_seed(0)
    idx = index.IndexFlatIP(768)
    idx.reserve(rows)
    for lo in range(0, rows, 1 << 18):
        idx.add(torch.randn((min(rows, lo + (1 << 18)) - lo, 768), generator=g, device=dev).cpu().numpy())
    ret = mhop.SyntheticTwoHop(idx, B, k, k, 768, dev)
    # QA arena: passages of 2-5 sentences, 60-250 WordPieces, ids in the ELECTRA vocabulary
    rng = np.random.default_rng(1)
    lens = rng.integers(60, 251, rows)
    ns = rng.integers(2, 6, rows)
    offs = np.zeros(rows + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    soffs = np.zeros(rows + 1, np.int64)
    soffs[1:] = np.cumsum(ns)
    owner = np.repeat(np.arange(rows), ns)  # sentence j of passage p starts at j * (len // n_sents): ascending, inside the passage
    starts = ((np.arange(int(soffs[-1])) - soffs[owner]) * (lens[owner] // ns[owner])).astype(np.int32)
    qa = qa_arena.QAArena(rng.integers(1000, 30000, int(offs[-1])).astype(np.int32), offs, starts, soffs).to(dev)
    cfg = transformers.ElectraConfig(vocab_size=30522, hidden_size=1024, embedding_size=1024, num_hidden_layers=24, num_attention_heads=16,
                                     intermediate_size=4096, max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12)
    m = reader.QAModel(cfg, types.SimpleNamespace(model_name="google/electra-large-discriminator", sp_pred=True))
    sd = {}
    for key, shp in m.state_dict().items():
        if key.endswith("LayerNorm.weight"):
            sd[key] = 1.0 + 0.1 * torch.randn(shp, generator=g, device=dev)
        elif key.endswith("bias") or "embeddings" in key:
            sd[key] = 0.1 * torch.randn(shp, generator=g, device=dev)
        else:
            sd[key] = (1.0 / shp[1] ** 0.5) * torch.randn(shp, generator=g, device=dev)
    m.load_state_dict(sd)
    m.to(dev)
    special = {"cls": 101, "sep": 102, "yes": 2748, "no": 2053, "pad": 0}
    corpus = synthetic_corpus(64, seed=2)
    qtok = transformers.BertTokenizer(VOCAB, do_lower_case=True)  # host decode: the toy WordPiece tokenizer on synthetic text
    q_len = 20
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    tot = {"retrieval": 0.0, "assembly": 0.0, "reader": 0.0, "host_decode": 0.0}
    for it in range(steps + 1):
        e = [ev() for _ in range(4)]
        e[0].record()
        out = ret.step()
        e[1].record()
        chains = torch.stack([out["hop1"], out["hop2"]], -1).reshape(-1, 2)
        row_q = torch.arange(B, device=dev).repeat_interleave(k)
        q_ids = torch.randint(1000, 30000, (B, q_len), device=dev)
        q_lens = torch.full((B,), q_len, dtype=torch.int64, device=dev)
        ch_host = chains.cpu().numpy()  # (the CLI's chains are on the host already: rank_paths)
        e1b = ev()
        e1b.record()
        L, S = qa.batch_shape([q_len] * B, ch_host, np.repeat(np.arange(B), k), 512)
        rows_t = qa_arena.assemble(qa, q_ids, q_lens, chains, row_q, special, 512, L, S)
        e[2].record()
        head = m.decode({kk: rows_t[kk] for kk in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets")}, 35)
        e[3].record()
        packed = torch.cat([head["start"].double()[:, None], head["end"].double()[:, None], head["span_score"].double()[:, None],
                            head["rank_score"].double().view(-1, 1)], 1).cpu()
        sp = head["sp_prob"].float().cpu().tolist()
        h0 = time.perf_counter()
        hl = {"start": [min(int(x), 40) for x in packed[:, 0]], "end": [min(int(x), 42) for x in packed[:, 1]], "span_score": packed[:, 2].tolist(),
              "rank_score": packed[:, 3].tolist(), "sp_prob": sp}
        items = [{"_id": f"q{b}", "question": "which film was released first?"} for b in range(B)]
        psg = [[[corpus[str((b + j) % 64)], corpus[str((b + j + 1) % 64)]] for j in range(k)] for b in range(B)]
        end2end.select_and_decode(items, hl, psg, [q_len + 2] * B, qtok, True)
        h1 = time.perf_counter()
        torch.cuda.synchronize()
        if it == 0:
            continue  # warm-up
        tot["retrieval"] += e[0].elapsed_time(e[1])
        tot["assembly"] += e1b.elapsed_time(e[2])
        tot["reader"] += e[2].elapsed_time(e[3])
        tot["host_decode"] += (h1 - h0) * 1e3
    ms = {key: v / steps for key, v in tot.items()}
    total = sum(ms.values())
    print(json.dumps({"leg": "e2e", "rows": rows, "batch": B, "topk": k, "ms_per_batch": {key: round(v, 3) for key, v in ms.items()},
                      "ms_per_question": round(total / B, 3), "questions_per_s": round(B / (total / 1e3), 1), "reader_rows": B * k,
                      "row_len": int(L), "steps": steps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--topks", default="1,2,5,10,20,50")
    ap.add_argument("--batches", default="1,100")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--one", default=None, help="BxK: one configuration in this process")
    ap.add_argument("--host", action="store_true", help="only the host-cost leg")
    a = ap.parse_args()
    if a.host:
        host_costs()
        return
    if a.one:
        B, k = map(int, a.one.split("x"))
        one(a.rows, B, k, a.steps)
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--host"], timeout=a.timeout)
    if r.returncode != 0:
        sys.exit(1)
    for B in map(int, a.batches.split(",")):
        for k in map(int, a.topks.split(",")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", f"{B}x{k}", "--rows", str(a.rows), "--steps", str(a.steps)],
                               timeout=a.timeout)
            if r.returncode != 0:
                print(f"end2end_bench: {B}x{k} exited with {r.returncode}; stopping", file=sys.stderr)
                sys.exit(1)


if __name__ == "__main__":
    main()
