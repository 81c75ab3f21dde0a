"""Generate tests/golden/reader_* by EXECUTING the reference's reader code (run once, where the reference checkout is present):

    python scripts/gen_reader_golden.py [--ref /path/to/multihop_dense_retrieval]

It imports mdr/qa/qa_dataset.py (QADataset, qa_collate), mdr/qa/qa_model.py (QAModel) and scripts/train_qa.py (predict, eval_final)
from the reference tree under stubs for what this environment lacks: transformers 2.11's `encode_plus(..., is_pretokenized=True)`
(the convention documented in multihop_dense_retrieval_amd/qa_data.py), `ujson` -> json, tensorboard, apex, `transformers.AdamW`.
Assets are toys: a tiny WordPiece vocab (with [unused0-2], yes, no), a seeded 1-layer ELECTRA (hidden 128, head dim 64, FFN 256, max_pos 512: one fp32 checkpoint under 1 MiB) and
HotpotQA-shaped items covering a truncated chain (sentence markers past max_seq_len), a question longer than max_q_len, trailing `?`,
yes / no gold answers, `##` pieces and accents in answer spans, and both --sp-pred settings.

Written: reader_electra_tiny/ (vocab.txt, config.json, items.jsonl, ckpt.pt with sp.*; the no-sp model is the same weights without sp.*), reader_batches.npz (the reference's collated
tensors and its fp32 head outputs per batch), reader_ref.json (wp_tokens / tok_to_orig_index / para_offsets per chain, the reference's
log lines and --save-prediction bytes of predict() and eval_final() fed its own model outputs, the fp32 model's span decisions).
"""
import argparse
import contextlib
import io
import json
import logging
import os
import random
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")

WORDS = ("the a of in and was is by for on at to from with as his her it an be born film album band city river state county "
         "director american british french actor singer writer player team season war king queen john paul george mary new york london "
         "paris berlin music rock pop 1990 2001 1876 first second largest capital founded released known called").split()
PIECES = ["##s", "##ed", "##ing", "##er", "##ly", "##a", "##o", "##e", "##i", "##n", "##t", "##r", "##l"]


def write_vocab(path):
    toks = ["[PAD]", "[unused0]", "[unused1]", "[unused2]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "yes", "no", ".", ",", "?", "'", "(", ")",
            "-", "cafe", "bjork", "zurich"] + WORDS + PIECES + list("abcdefghijklmnopqrstuvwxyz0123456789")
    seen, out = set(), []
    for t in toks:
        if t not in seen:
            seen.add(t)
            out.append(t)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    return out


def make_items(rng):
    def sent(n):
        return " ".join(rng.choice(WORDS) for _ in range(n)) + " ."

    def para(title, k, n=8):
        return {"title": title, "sents": [sent(n) for _ in range(k)]}

    items = []
    specs = [("q1", "which film was released first ?", ["Rock Film"], 3),
             ("q2", "was john born in paris", ["yes"], 2),
             ("q3", "is the city the capital", ["no"], 2),
             ("q4", " ".join(rng.choice(WORDS) for _ in range(90)) + "?", ["Café Zürich"], 3),
             ("q5", "who founded the band", ["Björk and Paul"], 4)]
    for qi, (qid, q, ans, nchains) in enumerate(specs):
        gold_a, gold_b = para(f"Gold {qid} A", 3), para(f"Gold {qid} B", 2)
        gold_a["sents"][1] = f"the answer is {ans[0]} playing loudly ."
        chains = [[gold_a, gold_b]]
        for c in range(nchains - 1):
            chains.append([para(f"Neg {qid} {c}", 2 + c), para(f"Neg {qid} {c} b", 2)])
        if qid == "q5":  # a long chain: markers past max_seq_len
            chains.append([para("Long one", 30, 12), para("Long two", 20, 12)])
        items.append({"_id": qid, "question": q, "answer": ans, "candidate_chains": chains,
                      "sp": [dict(gold_a, sp_sent_ids=[1]), dict(gold_b, sp_sent_ids=[0])], "type": "bridge"})
    return items


class Ref211Tokenizer:
    """transformers 2.11 surface the reference calls, on the WordPiece tokenizer of this environment."""

    def __init__(self, vocab):
        import transformers
        self.tok = transformers.BertTokenizer(vocab, do_lower_case=True)
        self.pad_token_id = self.tok.pad_token_id

    def tokenize(self, text):
        return self.tok.tokenize(text)

    def convert_tokens_to_ids(self, t):
        return self.tok.convert_tokens_to_ids(t)

    def encode_plus(self, q_toks, text_pair=None, max_length=None, return_tensors=None, is_pretokenized=False):
        assert is_pretokenized and return_tensors == "pt"
        toks = ["[CLS]"] + list(q_toks) + ["[SEP]"] + list(text_pair) + ["[SEP]"]
        assert len(toks) <= max_length
        ids = torch.tensor([self.tok.convert_tokens_to_ids(toks)])
        tt = torch.zeros_like(ids)
        tt[0, len(q_toks) + 2:] = 1
        return {"input_ids": ids, "token_type_ids": tt, "attention_mask": torch.ones_like(ids)}


def install_stubs():
    sys.modules["ujson"] = json
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = lambda *a, **k: None
    sys.modules["torch.utils.tensorboard"] = tb
    apex = types.ModuleType("apex")
    apex.amp = types.SimpleNamespace(register_half_function=lambda *a, **k: None, initialize=lambda m, *a, **k: m)
    sys.modules["apex"] = apex


class ListLogger:
    def __init__(self):
        self.lines = []

    def info(self, msg, *a):
        self.lines.append(msg % a if a else str(msg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MDR_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    install_stubs()
    sys.path.insert(0, a.ref)
    sys.path.insert(0, os.path.join(a.ref, "scripts"))
    import transformers
    from mdr.qa import qa_dataset as ref_ds
    from mdr.qa import qa_model as ref_model
    sys.modules["transformers"].AdamW = torch.optim.AdamW  # (the lazy module object in sys.modules is replaced as models are imported)
    import train_qa as ref_train

    os.makedirs(ASSETS, exist_ok=True)
    rng = random.Random(7)
    write_vocab(os.path.join(ASSETS, "vocab.txt"))
    cfg = transformers.ElectraConfig(vocab_size=len(open(os.path.join(ASSETS, "vocab.txt")).read().split("\n")) - 1, hidden_size=128,
                                     embedding_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256,
                                     max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12)
    cfg.save_pretrained(ASSETS)
    items = make_items(rng)
    with open(os.path.join(ASSETS, "items.jsonl"), "w") as f:
        for it in items:
            f.write(json.dumps(it) + "\n")
    tok = Ref211Tokenizer(os.path.join(ASSETS, "vocab.txt"))
    max_seq_len, max_q_len, bs = 160, 24, 4
    ds = ref_ds.QADataset(tok, os.path.join(ASSETS, "items.jsonl"), max_seq_len, max_q_len)
    batches = [ref_ds.qa_collate([ds[i] for i in range(lo, min(len(ds), lo + bs))], pad_id=tok.pad_token_id) for lo in range(0, len(ds), bs)]

    torch.manual_seed(0)
    transformers.AutoModel.from_pretrained = staticmethod(lambda name: transformers.ElectraModel(cfg))
    out_npz, ref = {}, {"max_seq_len": max_seq_len, "max_q_len": max_q_len, "batch_size": bs, "chains": [], "runs": {}}
    for b in batches:
        for i in range(len(b["qids"])):
            ref["chains"].append({"qid": b["qids"][i], "para_offset": b["para_offsets"][i], "wp_tokens": b["wp_tokens"][i],
                                  "tok_to_orig_index": b["tok_to_orig_index"][i], "doc_tokens": b["doc_tokens"][i]})
    for bi, b in enumerate(batches):
        for k, v in b["net_inputs"].items():
            out_npz[f"b{bi}.{k}"] = v.numpy()
    for sp_pred in (True, False):
        args = types.SimpleNamespace(model_name="electra-tiny", sp_weight=0.0, sp_pred=sp_pred, max_ans_len=35, save_prediction="")
        torch.manual_seed(1)
        model = ref_model.QAModel(cfg, args)
        if sp_pred:
            with torch.no_grad():  # O(1) sub-layer outputs, spread head logits
                for n, p in model.named_parameters():
                    if n.endswith("LayerNorm.weight"):
                        p.copy_(1.0 + 0.1 * torch.randn_like(p))
                    elif n.endswith("bias"):
                        p.copy_(0.1 * torch.randn_like(p))
                    elif "embeddings" in n:
                        p.copy_(0.5 * torch.randn_like(p))
                    else:
                        p.copy_((1.5 / p.shape[1] ** 0.5) * torch.randn_like(p))
            sd = model.state_dict()
            torch.save(sd, os.path.join(ASSETS, "ckpt.pt"))
        else:
            model.load_state_dict({k: v for k, v in sd.items() if not k.startswith("sp.")})
        tag = "sp" if sp_pred else "nosp"
        model.eval()
        model.train = lambda mode=True: model  # predict() ends with model.train()
        ref_train.move_to_cuda = lambda x: x
        for bi, b in enumerate(batches):
            with torch.no_grad():
                o = model(b["net_inputs"])
            for k, v in o.items():
                if v is not None:
                    out_npz[f"{tag}.b{bi}.{k}"] = v.numpy()
        run = {}
        for mode in ("predict", "eval_final"):
            path = os.path.join(ASSETS, f"_pred_{tag}_{mode}.json")
            args.save_prediction = path
            lg = ListLogger()
            with contextlib.redirect_stdout(io.StringIO()):
                if mode == "predict":
                    ref_train.predict(args, model, batches, lg, fixed_thresh=0.8)
                else:
                    ref_train.eval_final(args, model, batches, weight=0.8, gpu=False)
            run[mode] = {"log": lg.lines, "save_prediction": open(path).read()}
            os.remove(path)
        ref["runs"][tag] = run
    np.savez_compressed(os.path.join(GOLD, "reader_batches.npz"), **out_npz)
    with open(os.path.join(GOLD, "reader_ref.json"), "w") as f:
        json.dump(ref, f)
    print("chains", len(ref["chains"]), "batches", len(batches))


if __name__ == "__main__":
    logging.disable(logging.WARNING)
    main()
