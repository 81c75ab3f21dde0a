"""Generate tests/golden/reader_train_ref.npz by EXECUTING the reference's reader in training mode (run once, where the reference checkout
is present; the file regenerates byte for byte):

    python scripts/gen_reader_train_golden.py [--ref /path/to/multihop_dense_retrieval] [--out FILE]

It imports mdr/qa/qa_dataset.py (QADataset(train=True), qa_collate) and mdr/qa/qa_model.py (QAModel) from the reference tree under the stubs
of scripts/gen_reader_golden.py, loads the committed tiny ELECTRA (tests/golden/reader_electra_tiny: config, vocab, items.jsonl, ckpt.pt),
sets every dropout probability to 0, and runs QAModel.forward in train() mode and backward() on the CPU in fp32: batch 0 with --sp-pred
(sp_weight 0.5), batch 1 without. The training-branch fields (starts, ends, sent_labels, label) are the reference dataset's own.

Every chain of the committed items is longer than max_seq_len = 48 (the file must stay under 200 KB and holds position rows 0 .. L - 1), so
the script adds two short toy items of its own, t1 (a span answer) and t2 (yes), to a temporary copy of items.jsonl: the batches then hold
rows of different lengths and padding. The committed fixture is not changed.

The two batches (max_seq_len 48, max_q_len 24; picked from QADataset(train=True) by qid and label): b0 = the gold chain of q1 (a span
answer, cut at max_seq_len), the gold chain and the negative of t1 (short rows; the negative has starts = [-1]) and the gold chain of q2
(yes); b1 = the gold chain of q3 (no), the gold chain and the negative of t2, and the long negative of q5 (sentence markers behind the cut).

Written per set s in ("sp.b0", "nosp.b1"): s.in.<net input>, s.loss, s.out.<score tensor> (the eval-mode scores of the same weights: with
dropout 0 they are what the training branch saw), s.g.<name> for every 1-D gradient and the type table's in full,
s.g.encoder.embeddings.position_embeddings.weight rows 0 .. L - 1, s.rows.<word table> the ids that occur and s.g.<word table> their rows,
and for every other matrix s.norm.<name> (the fp64 Frobenius norm of the whole gradient) and s.g.<name> rows 0, ROW_STRIDE, 2 ROW_STRIDE, ...
"""
import argparse
import json
import logging
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")
MAX_SEQ_LEN, MAX_Q_LEN = 48, 24
ROW_STRIDE = 32
SP_WEIGHT = 0.5
WORD = "encoder.embeddings.word_embeddings.weight"
POS = "encoder.embeddings.position_embeddings.weight"
TYPE = "encoder.embeddings.token_type_embeddings.weight"
SETS = (("sp.b0", True, 0), ("nosp.b1", False, 1))


TOY_ITEMS = [
    {"_id": "t1", "question": "which city is the capital ?", "answer": ["London"], "type": "bridge",
     "sp": [{"title": "City one", "sents": ["the capital is london .", "it was founded first ."], "sp_sent_ids": [0]},
            {"title": "City two", "sents": ["paris is a city ."], "sp_sent_ids": [0]}],
     "candidate_chains": [[{"title": "River", "sents": ["the river is in berlin ."]}, {"title": "State", "sents": ["a state ."]}]]},
    {"_id": "t2", "question": "was the king born in york", "answer": ["yes"], "type": "comparison",
     "sp": [{"title": "King", "sents": ["the king was born in york ."], "sp_sent_ids": [0]}, {"title": "York", "sents": ["york is a city .", "a river ."], "sp_sent_ids": [1]}],
     "candidate_chains": [[{"title": "Queen", "sents": ["the queen ."]}, {"title": "War", "sents": ["the first war ."]}]]},
]
for _it in TOY_ITEMS:  # the gold chain is a candidate too, as in the reference's data (the dataset skips it among the negatives)
    _it["candidate_chains"].insert(0, [{k: v for k, v in p.items() if k != "sp_sent_ids"} for p in _it["sp"]])


def pick_batches(ds):
    """indices into the reference's QADataset(train=True), by qid and label: see the module docstring"""
    by = {}
    for i, d in enumerate(ds.data):
        by.setdefault(d["qid"], []).append(i)
    q1, q2, q3, q5, t1, t2 = (by[q] for q in ("q1", "q2", "q3", "q5", "t1", "t2"))
    assert all(ds.data[q[0]]["label"] == 1 and all(ds.data[i]["label"] == 0 for i in q[1:]) for q in (q1, q2, q3, q5, t1, t2))
    assert len(t1) == 2 and len(t2) == 2 and len(q5) == 5
    return [[q1[0]] + t1 + [q2[0]], [q3[0]] + t2 + [q5[-1]]]


def stored_gradients(grads, L, ids):
    """{key suffix: array}: the stored part of every gradient (module docstring)"""
    out = {}
    for name, g in grads.items():
        g = g.numpy()
        if g.ndim == 1 or name == TYPE:
            out["g." + name] = g
        elif name == POS:
            out["g." + name] = g[:L]
        elif name == WORD:
            rows = np.unique(ids)
            out["rows." + name] = rows.astype(np.int64)
            out["g." + name] = g[rows]
        else:
            out["norm." + name] = np.asarray(np.sqrt((g.astype(np.float64) ** 2).sum()))
            out["g." + name] = g[::ROW_STRIDE]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MDR_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(GOLD, "reader_train_ref.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_reader_golden as g
    g.install_stubs()
    sys.path.insert(0, a.ref)
    import transformers
    from mdr.qa import qa_dataset as ref_ds
    from mdr.qa import qa_model as ref_model

    torch.manual_seed(0)
    torch.set_num_threads(1)  # one summation order: the file regenerates byte for byte
    cfg = transformers.ElectraConfig.from_pretrained(ASSETS)
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = 0.0
    tok = g.Ref211Tokenizer(os.path.join(ASSETS, "vocab.txt"))
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "items.jsonl"), "w") as f:
            f.write(open(os.path.join(ASSETS, "items.jsonl")).read())
            for it in TOY_ITEMS:
                f.write(json.dumps(it) + "\n")
        ds = ref_ds.QADataset(tok, os.path.join(tmp, "items.jsonl"), MAX_SEQ_LEN, MAX_Q_LEN, train=True)
    batches = [ref_ds.qa_collate([ds[i] for i in idx], pad_id=tok.pad_token_id)["net_inputs"] for idx in pick_batches(ds)]
    transformers.AutoModel.from_pretrained = staticmethod(lambda name: transformers.ElectraModel(cfg))
    sd = torch.load(os.path.join(ASSETS, "ckpt.pt"), map_location="cpu")
    out = {}
    for tag, sp_pred, bi in SETS:
        args = types.SimpleNamespace(model_name="electra-tiny", sp_weight=SP_WEIGHT, sp_pred=sp_pred)
        model = ref_model.QAModel(cfg, args)
        own = dict(model.named_parameters())
        missing = [k for k in own if k not in sd]
        assert not missing, missing
        model.load_state_dict({k: v for k, v in sd.items() if sp_pred or not k.startswith("sp.")}, strict=False)
        batch = batches[bi]
        assert batch["input_ids"].shape[1] <= MAX_SEQ_LEN and {"starts", "ends", "sent_labels", "label", "token_type_ids"} <= set(batch)
        model.train()
        loss = model(batch)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in own.items()}
        assert all(bool(torch.isfinite(v).all()) for v in grads.values()) and float(grads[POS][0].abs().max()) > 0
        model.eval()
        with torch.no_grad():
            scores = model(batch)
        for k, v in batch.items():
            out[f"{tag}.in.{k}"] = v.numpy()
        out[f"{tag}.loss"] = loss.detach().numpy()
        for k, v in scores.items():
            if v is not None:
                out[f"{tag}.out.{k}"] = v.numpy()
        for k, v in stored_gradients(grads, batch["input_ids"].shape[1], batch["input_ids"].numpy()).items():
            out[f"{tag}.{k}"] = v
        print(tag, "B, L =", tuple(batch["input_ids"].shape), "loss", float(loss.detach()), "starts", batch["starts"].tolist(), "label", batch["label"].reshape(-1).tolist(),
              "lengths", batch["attention_mask"].sum(1).tolist())
    out["meta.max_seq_len"], out["meta.max_q_len"], out["meta.row_stride"] = np.asarray(MAX_SEQ_LEN), np.asarray(MAX_Q_LEN), np.asarray(ROW_STRIDE)
    out["meta.sp_weight"] = np.asarray(SP_WEIGHT, np.float32)
    np.savez_compressed(a.out, **{k: out[k] for k in sorted(out)})
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    logging.disable(logging.WARNING)
    main()
