"""Generate tests/golden/mhop_eval_ref.{json,npz} by EXECUTING the reference's scripts/train_mhop.py --do_predict (run once, where the
reference checkout is present):

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_mhop_eval_golden.py [--ref /path/to/multihop_dense_retrieval]

The script runs as __main__ (runpy.run_path) on toy assets, in fp32 with --num_workers 0 (apex does not exist here, so no O1 run can be
captured: the fp16 rounding points of the product are pinned by the exact-grid GPU tests instead). The library stubs and the
transformers-2.11 tokenizer adapter are IMPORTED from oracle/gen_cli_golden.py (apex / tqdm / cuda no-ops, `encode_plus` with the 2.11
template and truncation); on top of them only a TensorBoard stub (the script opens a SummaryWriter even for --do_predict) and the
adapter's `pad_token_id` are added here. What the reference computed is captured by wrapping three of its own functions:
    mhop_collate            the collated tensors of every batch
    RobertaRetriever.forward  the six fp32 embedding matrices of every batch
    mhop_eval               rrs_1 / rrs_2 of every batch
plus its log lines (stderr) and, from the imported mhop_loss fed the captured outputs, the loss value of every batch.

Toy assets (`build_assets`, shared with the tests: it needs numpy / torch / transformers and tests/golden/tiny_bpe, not the reference):
a 2-layer 128-wide RoBERTa with seeded weights and a `module.`-prefixed checkpoint; 24 dev samples -- every third one a comparison
question (the order of its positives is the reference's random.shuffle under --seed), questions with and without a trailing "?", one
passage far longer than --max_c_len, question + passage pairs longer than --max_q_sp_len, samples whose bridge passage comes first
in `pos_paras`, a sample with three negatives. Questions repeat words of their start passage and bridge passages repeat words of
the hop-2 query, so that most targets win by a margin (the share of ranks a device run cannot be held to is reported and asserted
<= 10 %, see `decided`). Only data is written.
"""
import argparse
import contextlib
import io
import json
import logging
import os
import runpy
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED, N_SAMPLES, BATCH = 16, 24, 4
MAX_Q_LEN, MAX_Q_SP_LEN, MAX_C_LEN = 14, 30, 40
WEIGHT_SEED = 29
# largest elementwise embedding error assumed for a device run when the generator checks the decided share on the CPU: the tiny geometry's
# fixture bar of tests/test_encoder_gpu.py (max |err| <= 6e-3 on unit-scale outputs)
ASSUMED_ELEM_ERR = 6e-3
KEYS = ("q", "q_sp1", "c1", "c2", "neg_1", "neg_2")


def dev_samples():
    from oracle import seeded
    words = ("the quick brown fox jumps over lazy dog river bank retrieval encoder index beam passage question answer Paris London film band "
             "album studio producer capital France Seine stadium people author born city population 1950 2012 80,000 3.14").split()
    pick = seeded.integers(SEED, "mhop.words", (N_SAMPLES * 6, 64), 0, len(words))
    lens = seeded.integers(SEED, "mhop.lens", (N_SAMPLES * 6,), 6, 24)

    def text(r, n=None):
        return " ".join(words[j] for j in pick[r, :(n or lens[r])])

    out = []
    for i in range(N_SAMPLES):
        start_text, bridge_tail = text(6 * i), text(6 * i + 1)
        q_words = start_text.split()[:6 + i % 5] + text(6 * i + 2, 1 + i % 2).split()
        question = " ".join(q_words) + ("" if i % 7 == 3 else "?")
        # the bridge passage repeats the question and the head of the start passage: close to the hop-2 query (question + start text)
        bridge_text = " ".join(q_words + start_text.split()[:10]) + " " + " ".join(bridge_tail.split()[:6])
        if i == 5:
            start_text = " ".join([start_text] * 12)  # far beyond --max_c_len and --max_q_sp_len
        start = {"title": f"Start {i} " + " ".join(q_words[:2]), "text": start_text + ("  " if i % 4 == 1 else "")}
        bridge = {"title": f"Bridge {i}", "text": bridge_text}
        comparison = i % 3 == 0
        s = {"question": question, "type": "comparison" if comparison else "bridge",
             "pos_paras": [bridge, start] if i % 2 else [start, bridge],
             "neg_paras": [{"title": f"Neg {i}.{n}", "text": text(6 * i + 3 + n)} for n in range(3 if i == 2 else 2)]}
        if not comparison:
            s["bridge"] = bridge["title"]
        out.append(s)
    return out


def build_assets(out_dir):
    """Writes the toy model directory, checkpoint and dev file under out_dir; returns their paths and the in-memory pieces."""
    import torch
    import transformers
    from oracle import gen_cli_golden as cli
    from oracle import seeded
    os.makedirs(out_dir, exist_ok=True)
    tok = cli.tiny_tokenizer()
    geom = dict(seeded.TINY, vocab=max(seeded.TINY["vocab"], len(tok)))
    sd = seeded.make_state_dict(WEIGHT_SEED, geom)
    # A random-weight encoder gives every sequence nearly the same [CLS] vector (cosines 0.9+: the <s> embedding at position 2 dominates),
    # so that all scores of a row sit within 1 % of each other. Damp the input rows every sequence shares; the embeddings then differ
    # (cosines 0.7-0.85) and the targets of related texts win by a margin. Everything else keeps the scales of oracle/seeded.py, the
    # regime the encoder's fixture bar (tests/test_encoder_gpu.py) was set for.
    sd["encoder.embeddings.word_embeddings.weight"][0] *= 0.3
    sd["encoder.embeddings.position_embeddings.weight"][2] *= 0.3
    sd["encoder.embeddings.token_type_embeddings.weight"][:] *= 0.3
    model_dir = os.path.join(out_dir, "toy-roberta-tiny")
    cfg = transformers.RobertaConfig(vocab_size=geom["vocab"], hidden_size=geom["hidden"], num_hidden_layers=geom["layers"],
                                     num_attention_heads=geom["heads"], intermediate_size=geom["ffn"], max_position_embeddings=514, type_vocab_size=1,
                                     layer_norm_eps=1e-5, pad_token_id=1, bos_token_id=0, eos_token_id=2, hidden_act="gelu")
    cfg.save_pretrained(model_dir)
    tok.save_pretrained(model_dir)
    ckpt = os.path.join(out_dir, "q_encoder_tiny.pt")
    torch.save({"module." + k: torch.from_numpy(v) for k, v in sd.items()}, ckpt)
    samples = dev_samples()
    dev = os.path.join(out_dir, "dev.jsonl")
    with open(dev, "w") as f:
        f.write("\n".join(json.dumps(s) for s in samples))
    return {"tok": tok, "geom": geom, "sd": sd, "model_dir": model_dir, "ckpt": ckpt, "dev": dev, "samples": samples}


def cli_argv(a, extra=()):
    return ["--do_predict", "--predict_batch_size", str(BATCH), "--model_name", a["model_dir"], "--predict_file", a["dev"], "--init_checkpoint", a["ckpt"],
            "--seed", str(SEED), "--max_c_len", str(MAX_C_LEN), "--max_q_len", str(MAX_Q_LEN), "--max_q_sp_len", str(MAX_Q_SP_LEN), "--shared-encoder",
            "--num_workers", "0"] + list(extra)


def score_matrices(emb):
    """The two [B, 2B + 2] fp64 score matrices of one batch (column B + i of hop-1 row i is -inf) and the column norms, from fp32 embeddings."""
    e = {k: np.asarray(emb[k], np.float64) for k in KEYS}
    B = e["q"].shape[0]
    ctx = np.concatenate([e["c1"], e["c2"]])
    out = []
    for qk in ("q", "q_sp1"):
        s = np.concatenate([e[qk] @ ctx.T, (e[qk] * e["neg_1"]).sum(1)[:, None], (e[qk] * e["neg_2"]).sum(1)[:, None]], axis=1)
        cn = np.concatenate([np.broadcast_to(np.linalg.norm(ctx, axis=1), (B, 2 * B)), np.linalg.norm(e["neg_1"], axis=1)[:, None],
                             np.linalg.norm(e["neg_2"], axis=1)[:, None]], axis=1)
        out.append((s, cn, np.linalg.norm(e[qk], axis=1)))
    out[0][0][np.arange(B), B + np.arange(B)] = -np.inf
    return out


def decided(emb, elem_err, score_slack=0.0):
    """Which ranks of one batch a run with perturbed embeddings is held to: [2, B] bool. `elem_err[k]` is the largest elementwise error of matrix k.
    A score q.c moves by dq.c + q.dc; the elementwise errors are rounding noise of the encoder, not aligned with the other operand, so each term is
    of the order (rms error) x |row|. The threshold uses the LARGEST elementwise error in place of the rms one (3-4 x larger on the tiny geometry:
    3.0e-3 against 6.6e-4..9e-4): move(i, j) = err_q |c_j| + err_c |q_i|, a several-sigma allowance, not a worst-case bound (Cauchy-Schwarz would
    put sqrt(d) on top and decide almost nothing). A rank is decided when the target's score is further from EVERY other finite score of its row
    than the allowances of the two scores together. `score_slack`: a further absolute allowance per score (the fp16 rounding of a score under --fp16)."""
    e = {k: np.asarray(emb[k], np.float64) for k in KEYS}
    B = e["q"].shape[0]
    ones = np.ones(B)
    cerr = np.concatenate([elem_err["c1"] * ones, elem_err["c2"] * ones])
    res = np.zeros((2, B), bool)
    for h, ((s, cn, qn), qk) in enumerate(zip(score_matrices(emb), ("q", "q_sp1"))):
        ce = np.concatenate([np.broadcast_to(cerr, (B, 2 * B)), elem_err["neg_1"] * ones[:, None], elem_err["neg_2"] * ones[:, None]], axis=1)
        move = elem_err[qk] * cn + qn[:, None] * ce
        t = np.arange(B) + h * B
        gap = np.abs(s - s[np.arange(B), t][:, None])
        need = move + move[np.arange(B), t][:, None] + 2 * score_slack
        ok = (gap > need) | ~np.isfinite(s)
        ok[np.arange(B), t] = True
        res[h] = ok.all(1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MDR_REFERENCE", "/root/reference"))
    ref_root = ap.parse_args().ref
    import warnings
    warnings.simplefilter("ignore")
    import torch
    import transformers
    from oracle import gen_cli_golden as cli
    cli.REF = ref_root
    script = os.path.join(ref_root, "scripts", "train_mhop.py")
    tmp = tempfile.mkdtemp(prefix="mdr_mhop_eval_golden_")
    a = build_assets(tmp)
    # AutoModel.from_pretrained(--model_name) (mhop_retriever.py:20) wants weights next to the config; load_saved then overwrites every one of them
    transformers.RobertaModel(transformers.AutoConfig.from_pretrained(a["model_dir"])).save_pretrained(a["model_dir"])
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = lambda *x, **k: None
    sys.modules["torch.utils.tensorboard"] = tb
    cli.RobertaTokenizer211.pad_token_id = property(lambda self: self.tok.pad_token_id)

    batches, embeds, rrs = [], [], []
    cap, err = cli.Capture(), io.StringIO()
    root_logger = logging.getLogger()
    root_logger.handlers.clear()
    with cli.stubbed(cap), contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        sys.modules["transformers"].AdamW = torch.optim.AdamW
        import mdr.retrieval.criterions as ref_crit
        import mdr.retrieval.data.mhop_dataset as ref_ds
        import mdr.retrieval.models.mhop_retriever as ref_model
        real = (ref_ds.mhop_collate, ref_model.RobertaRetriever.forward, ref_crit.mhop_eval)

        def collate(samples, pad_id=0):
            b = real[0](samples, pad_id=pad_id)
            batches.append({k: v.numpy().copy() for k, v in b.items()})
            return b

        def forward(self, batch):
            o = real[1](self, batch)
            embeds.append({k: v.detach().float().numpy().copy() for k, v in o.items()})
            return o

        def mhop_eval(outputs, args):
            r = real[2](outputs, args)
            rrs.append({k: list(v) for k, v in r.items()})
            return r

        ref_ds.mhop_collate, ref_model.RobertaRetriever.forward, ref_crit.mhop_eval = collate, forward, mhop_eval
        try:
            sys.argv = [script] + cli_argv(a, ["--output_dir", os.path.join(tmp, "logs")])
            runpy.run_path(script, run_name="__main__")
            losses = [float(ref_crit.mhop_loss(lambda batch, o=o: {k: torch.from_numpy(v) for k, v in o.items()}, None,
                                               types.SimpleNamespace(momentum=False)).item()) for o in embeds]
        finally:
            ref_ds.mhop_collate, ref_model.RobertaRetriever.forward, ref_crit.mhop_eval = real
    root_logger.handlers.clear()
    log = [ln for ln in err.getvalue().split("\n") if ln and "Loading weights" not in ln]
    n_batches = -(-N_SAMPLES // BATCH)
    assert len(batches) == len(embeds) == len(rrs) == n_batches, (len(batches), len(embeds), len(rrs))

    # the fixture's own scores must not tie (the reference's argsort is not stable: a tie would make its rank an accident of the sort)
    share = []
    for o in embeds:
        for s, _, _ in score_matrices({k: o[k] for k in KEYS}):
            for row in s:
                fin = row[np.isfinite(row)]
                assert len(np.unique(fin.astype(np.float32))) == len(fin), "two columns of one row tie in fp32: change WEIGHT_SEED"
        share.append(decided(o, {k: ASSUMED_ELEM_ERR for k in KEYS}))
    dec = np.concatenate(share, axis=1)
    excluded = 1.0 - dec.mean()
    print(f"ranks a device run is not held to at an elementwise embedding error of {ASSUMED_ELEM_ERR}: {int((~dec).sum())} of {dec.size} ({excluded:.1%})")
    assert excluded <= 0.10, "more than 10 % of the ranks are undecided under the assumed embedding error: change the samples or WEIGHT_SEED"

    perf_line = [ln for ln in log if "test performance" in ln][0]
    meta = {"generator": "scripts/gen_mhop_eval_golden.py: the reference's scripts/train_mhop.py --do_predict executed as __main__ under library stubs",
            "seed": SEED, "n_samples": N_SAMPLES, "batch": BATCH, "max_q_len": MAX_Q_LEN, "max_q_sp_len": MAX_Q_SP_LEN, "max_c_len": MAX_C_LEN,
            "weight_seed": WEIGHT_SEED, "n_batches": n_batches, "samples": a["samples"],
            "log": [ln.replace(tmp, "<assets>") for ln in log if " - __main__ - " in ln and "Namespace(" not in ln],
            "rrs_1": [r["rrs_1"] for r in rrs], "rrs_2": [r["rrs_2"] for r in rrs], "mhop_loss": losses,
            "test_performance": perf_line.split("test performance ", 1)[1],
            "assumed_elem_err": ASSUMED_ELEM_ERR, "undecided_share_at_assumed_err": excluded}
    arrays = {}
    for bi, (b, o) in enumerate(zip(batches, embeds)):
        for k, v in b.items():
            arrays[f"b{bi}.{k}"] = v.astype(np.int32)
        for k in KEYS:
            arrays[f"b{bi}.emb.{k}"] = o[k]
    with open(os.path.join(GOLD, "mhop_eval_ref.json"), "w") as f:
        json.dump(meta, f, indent=1)
    np.savez_compressed(os.path.join(GOLD, "mhop_eval_ref.npz"), **arrays)
    print("\n".join(meta["log"]))
    print("rrs_1", meta["rrs_1"], "\nrrs_2", meta["rrs_2"], "\nloss", losses)
    for n in ("mhop_eval_ref.json", "mhop_eval_ref.npz"):
        print(n, os.path.getsize(os.path.join(GOLD, n)), "bytes")


if __name__ == "__main__":
    main()
