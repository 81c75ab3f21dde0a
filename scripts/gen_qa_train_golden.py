"""Generate tests/golden/qa_train_ref.{npz,json} by EXECUTING the reference's reader training code (run once, where the reference checkout
is present; both files regenerate byte for byte):

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_qa_train_golden.py [--ref /path/to/multihop_dense_retrieval]

Under the stubs of scripts/gen_reader_golden.py (the transformers-2.11 tokenizer surface, apex, ujson) plus a TensorBoard writer that accepts
add_scalar, a silent tqdm, an identity move_to_cuda, and torch.optim.AdamW standing in for transformers.AdamW, it runs on the CPU in fp32:

  1. mdr/qa/qa_dataset.py QADataset(train=True) on tests/golden/qa_train_items.jsonl (authored for this project: the toy train file whose
     cases DESIGN.md §27 lists) with the tokenizer of tests/golden/reader_electra_tiny, max_seq_len 48, max_q_len 24: every item's fields;
  2. MhopSampler(num_neg=2): its len and the index sequences of three consecutive epochs under random.seed(SEED);
  3. qa_collate's net_inputs of every batch of the first of those epochs at batch size 4;
  4. scripts/train_qa.py --do_train as __main__ (runpy) on the same file as train and dev set, from reader_electra_tiny/ckpt.pt, both dropout
     probabilities 0: its __main__ log lines, the loss of every training batch (QAModel.forward wrapped), the index sequence its sampler
     drew, and the keys and shapes of the state dict it trains (and whether it wrote checkpoint_best.pt: it saves only when em improves).

The assertions at the end check that the toy file shows every case it was authored for, on the REFERENCE's output.
"""
import argparse
import contextlib
import io
import json
import logging
import os
import random
import runpy
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")
ITEMS = os.path.join(GOLD, "qa_train_items.jsonl")
MAX_SEQ_LEN, MAX_Q_LEN, SEED, NEG_NUM, BATCH = 48, 24, 5, 2, 4
EPOCHS, LR, EVAL_PERIOD, WARMUP, SP_WEIGHT = 3, 1e-3, 4, 0.1, 0.5
ITEM_FIELDS = ("input_ids", "token_type_ids", "attention_mask", "paragraph_mask", "starts", "ends", "sent_offsets", "sent_labels", "ans_covered", "label")


def train_argv(model_dir, ckpt, out_dir, extra=()):
    return ["--do_train", "--prefix", "toy", "--model_name", model_dir, "--train_file", ITEMS, "--predict_file", ITEMS, "--init_checkpoint", ckpt,
            "--seed", str(SEED), "--max_seq_len", str(MAX_SEQ_LEN), "--max_q_len", str(MAX_Q_LEN), "--train_batch_size", str(BATCH),
            "--predict_batch_size", "8", "--neg-num", str(NEG_NUM), "--num_workers", "0", "--num_train_epochs", str(EPOCHS), "--learning_rate", str(LR),
            "--warmup-ratio", str(WARMUP), "--eval-period", str(EVAL_PERIOD), "--sp-pred", "--sp-weight", str(SP_WEIGHT), "--output_dir", out_dir] + list(extra)


def item_fields(it):
    enc = it["encodings"]
    out = {k: enc[k].view(-1) for k in ("input_ids", "token_type_ids", "attention_mask")}
    out.update({k: it[k].view(-1) for k in ITEM_FIELDS[3:]})
    return {k: v.numpy().astype(np.int64) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MDR_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    import warnings
    warnings.simplefilter("ignore")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_reader_golden as g
    g.install_stubs()

    class Writer:
        def __init__(self, *x, **k):
            pass

        def add_scalar(self, *x, **k):
            pass

    sys.modules["torch.utils.tensorboard"].SummaryWriter = Writer
    sys.path.insert(0, a.ref)
    os.environ["TQDM_DISABLE"] = "1"  # no progress bars in the captured stderr
    import transformers
    from mdr.qa import qa_dataset as ref_ds
    from mdr.qa import qa_model as ref_model
    from mdr.qa import utils as ref_utils
    sys.modules["transformers"].AdamW = torch.optim.AdamW
    torch.set_num_threads(1)  # one summation order: the files regenerate byte for byte

    tok = g.Ref211Tokenizer(os.path.join(ASSETS, "vocab.txt"))
    arrays, meta = {}, {"generator": "scripts/gen_qa_train_golden.py: the reference's QADataset(train=True), MhopSampler, qa_collate and scripts/train_qa.py "
                                     "--do_train executed under library stubs", "max_seq_len": MAX_SEQ_LEN, "max_q_len": MAX_Q_LEN, "seed": SEED,
                        "neg_num": NEG_NUM, "batch": BATCH}
    with contextlib.redirect_stdout(io.StringIO()):
        ds = ref_ds.QADataset(tok, ITEMS, MAX_SEQ_LEN, MAX_Q_LEN, train=True)
        items = [item_fields(ds[i]) for i in range(len(ds))]
        records = [{"qid": d["qid"], "label": int(d["label"]), "para_offset": int(d["para_offset"]), "n_wp": len(d["wp_tokens"]),
                    "n_wp_uncut": len(d["context_processed"]["all_doc_tokens"]), "n_sent_uncut": len(d["context_processed"]["sent_starts"])} for d in ds.data]
        # match_answer_span returns list(set(...)): with two distinct surface strings the order of an item's spans would change from
        # process to process, and so would this file. The toy file has at most one per item.
        assert all(len(ref_utils.match_answer_span(d["context_processed"]["context"], d["gold_answer"], ds.simple_tok)) <= 1 for d in ds.data)
        ds = ref_ds.QADataset(tok, ITEMS, MAX_SEQ_LEN, MAX_Q_LEN, train=True)  # a fresh one: __getitem__ writes tensors into its records
    for i, it in enumerate(items):
        for k, v in it.items():
            arrays[f"item{i}.{k}"] = v
    meta["items"] = records
    meta["qid2gold"], meta["qid2neg"] = {k: list(v) for k, v in ds.qid2gold.items()}, {k: list(v) for k, v in ds.qid2neg.items()}
    random.seed(SEED)
    sampler = ref_ds.MhopSampler(ds, num_neg=NEG_NUM)
    meta["sampler_len"] = len(sampler)
    meta["epochs"] = [list(iter(sampler)) for _ in range(3)]
    first = meta["epochs"][0]
    meta["loader_len"] = len(torch.utils.data.DataLoader(ds, batch_size=BATCH, sampler=sampler))
    for bi, lo in enumerate(range(0, len(first), BATCH)):
        net = ref_ds.qa_collate([ds[i] for i in first[lo:lo + BATCH]], pad_id=tok.pad_token_id)["net_inputs"]
        for k, v in net.items():
            arrays[f"b{bi}.{k}"] = v.numpy().astype(np.int64)
    meta["n_batches"] = bi + 1

    # ---- the reference's scripts/train_qa.py --do_train as __main__ ------------------------------------------------------------------------
    tmp = tempfile.mkdtemp(prefix="mdr_qa_train_golden_")
    model_dir = os.path.join(tmp, "electra-tiny")  # QAModel looks for "electra" in --model_name
    os.makedirs(model_dir)
    shutil.copy(os.path.join(ASSETS, "vocab.txt"), model_dir)
    cfg_json = json.load(open(os.path.join(ASSETS, "config.json")))
    cfg_json["hidden_dropout_prob"], cfg_json["attention_probs_dropout_prob"] = 0.0, 0.0
    json.dump(cfg_json, open(os.path.join(model_dir, "config.json"), "w"), indent=1)
    cfg = transformers.ElectraConfig.from_pretrained(model_dir)
    script = os.path.join(a.ref, "scripts", "train_qa.py")
    out_dir = os.path.join(tmp, "logs")
    losses, drawn, state = [], [], {}
    real_forward, real_iter, real_cuda = ref_model.QAModel.forward, ref_ds.MhopSampler.__iter__, ref_utils.move_to_cuda
    real_tok, real_model = transformers.AutoTokenizer.from_pretrained, transformers.AutoModel.from_pretrained

    def forward(self, batch):
        out = real_forward(self, batch)
        if self.training:
            losses.append(float(out.detach().item()))
            state["sd"] = self
        return out

    def sampler_iter(self):
        idx = list(real_iter(self))
        drawn.append(idx)
        return iter(idx)

    err = io.StringIO()
    logging.getLogger().handlers.clear()
    ref_model.QAModel.forward, ref_ds.MhopSampler.__iter__, ref_utils.move_to_cuda = forward, sampler_iter, (lambda x: x)
    transformers.AutoTokenizer.from_pretrained = staticmethod(lambda name, *x, **k: g.Ref211Tokenizer(os.path.join(name, "vocab.txt")))
    transformers.AutoModel.from_pretrained = staticmethod(lambda name, *x, **k: transformers.ElectraModel(cfg))
    argv = sys.argv
    try:
        with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
            sys.argv = [script] + train_argv(model_dir, os.path.join(ASSETS, "ckpt.pt"), out_dir)
            runpy.run_path(script, run_name="__main__")
    finally:
        sys.argv = argv
        ref_model.QAModel.forward, ref_ds.MhopSampler.__iter__, ref_utils.move_to_cuda = real_forward, real_iter, real_cuda
        transformers.AutoTokenizer.from_pretrained, transformers.AutoModel.from_pretrained = real_tok, real_model
        logging.getLogger().handlers.clear()
    log = [ln.split(" - __main__ - ", 1)[1] for ln in err.getvalue().split("\n") if " - __main__ - " in ln and "Namespace(" not in ln]
    best = [os.path.join(dp, f) for dp, _, fs in os.walk(out_dir) for f in fs if f == "checkpoint_best.pt"]
    sd = state["sd"].state_dict()
    n_rows = [len(e) for e in drawn]
    per_epoch = [-(-n // BATCH) for n in n_rows]
    assert len(losses) == sum(per_epoch) and len(drawn) == EPOCHS, (len(losses), per_epoch)
    means, lo = [], 0
    for n in per_epoch:
        means.append(float(np.mean(losses[lo:lo + n])))
        lo += n
    assert means[-1] < means[0], ("the reference's own epoch means do not fall", means)
    meta["train"] = {"argv": [x.replace(ITEMS, "<items>") for x in train_argv("<model>", "<ckpt>", "<out>")], "epochs": EPOCHS, "learning_rate": LR, "eval_period": EVAL_PERIOD, "warmup_ratio": WARMUP,
                     "sp_weight": SP_WEIGHT, "log": [ln.replace(tmp, "<assets>").replace(ROOT, "<repo>") for ln in log], "loss": losses, "drawn": drawn, "epoch_means": means,
                     "state_dict": [[k, list(v.shape)] for k, v in sd.items() if "position_ids" not in k],
                     "checkpoint_best_written": bool(best), "checkpoint_best": [[k, list(v.shape)] for k, v in torch.load(best[0], map_location="cpu").items()] if best else None}
    shutil.rmtree(tmp)

    # ---- the cases the toy file was authored for, on the reference's output ----------------------------------------------------------------
    st = [it["starts"].tolist() for it in items]
    en = [it["ends"].tolist() for it in items]
    rec = records
    assert len(meta["qid2gold"]) % 8 == 1  # the multiple-of-8 cut drops a question
    assert any(len(s) == 3 for s in st)  # a span that occurs three times
    assert any(r["label"] == 1 and s != [-1] and e[0] == r["para_offset"] + r["n_wp"] - 1 and r["n_wp"] < r["n_wp_uncut"] and r["qid"] == "t2"
               for r, s, e in zip(rec, st, en))  # an end clamped to the last kept token
    assert any(r["label"] == 1 and s == [-1] for r, s in zip(rec, st))  # a gold chain whose span is wholly behind the cut
    assert any(r["label"] == 0 and int(it["ans_covered"][0]) == 1 and s != [-1] for r, it, s in zip(rec, items, st))  # distant supervision
    assert any(r["label"] == 0 and int(it["ans_covered"][0]) == 0 and r["qid"] == "t9" for r, it in zip(rec, items))
    assert any(len(it["sent_offsets"]) < r["n_sent_uncut"] for r, it in zip(rec, items))  # sentence markers behind the cut
    negs = [len(v) for v in meta["qid2neg"].values()]
    assert min(negs) < NEG_NUM < max(negs)
    assert meta["sampler_len"] == 8 * (NEG_NUM + 1) and all(len(e) < meta["sampler_len"] for e in meta["epochs"])

    with open(os.path.join(GOLD, "qa_train_ref.json"), "w") as f:
        json.dump(meta, f, indent=1)
    # (np.savez_compressed stamps no time into its members: the bytes are a function of the arrays)
    np.savez_compressed(os.path.join(GOLD, "qa_train_ref.npz"), **{k: arrays[k] for k in sorted(arrays)})
    print("\n".join(meta["train"]["log"]))
    print("loss", [round(x, 3) for x in losses])
    print("epoch means", means, "rows per epoch", n_rows, "sampler len", meta["sampler_len"], "loader len", meta["loader_len"])
    for n in ("qa_train_ref.json", "qa_train_ref.npz"):
        print(n, os.path.getsize(os.path.join(GOLD, n)), "bytes")


if __name__ == "__main__":
    main()
