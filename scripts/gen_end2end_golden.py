"""Generate tests/golden/end2end_ref.{json,npz} by EXECUTING the reference's scripts/end2end.py (run once, where the reference checkout is present):

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_end2end_golden.py [--ref /path/to/multihop_dense_retrieval]

The script runs as the module `scripts.end2end` (runpy.run_module, the reference root and its mdr/ first on sys.path) so that its
`from .train_qa import eval_final` resolves. Stubs and toy assets are IMPORTED from oracle/gen_cli_golden.py (tokenizer adapter with
transformers 2.11's batch_encode_plus, apex / tqdm / cuda no-ops) and scripts/gen_reader_golden.py (the is_pretokenized encode_plus
adapter, tensorboard / apex stubs); only what end2end.py needs on top is here:
  faiss.read_index   an exact index over the corpus rows augmented with one column (as the HNSW index is); `search` returns the NEGATED
                     inner product, best first, ties by ascending id. The query column convert_hnsw_query adds is 0, so the script's
                     `-(scores_1 + scores_2)` ranks by the same D + D' as the product.
  AutoConfig / AutoTokenizer / AutoModel   'roberta-base' -> the toy RoBERTa of gen_cli_golden.build_assets, 'google/electra-large-discriminator'
                     -> the toy ELECTRA and WordPiece vocabulary of tests/golden/reader_electra_tiny (load_saved overwrites the weights).
Corpus: the toy corpus of build_assets with a `sents` field added deterministically (corpus_with_sents) and every empty text replaced by
its title, so the script's inverted empty-passage rule is never reached. Questions: the first five (`readlines()[:5]` cuts nothing).

Captured per case: the chains as passage ids and their path scores, the reader's collated tensors per batch and its fp32 head outputs,
the log lines (stderr), the printed lines (the elapsed time blanked) and the --save-prediction bytes. Only data is written.
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
READER = os.path.join(GOLD, "reader_electra_tiny")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = [("k1_b1", ["--topk", "1", "--batch-size", "1"]), ("k3_b2_sp", ["--topk", "3", "--batch-size", "2", "--sp-pred"]), ("k4", ["--topk", "4"])]


def corpus_with_sents(docs):
    """{str(i): {"title", "text", "sents"}}: empty texts become their title; sentences of up to 7 words each."""
    out = {}
    for i, d in enumerate(docs):
        text = d["text"] if d["text"].strip() else d["title"]
        words = text.split()
        out[str(i)] = {"title": d["title"], "text": text, "sents": [" ".join(words[j:j + 7]) for j in range(0, len(words), 7)]}
    return out


def write_inputs(a, out_dir):
    """The corpus dict with sentences and the five questions the cases read; returns their paths."""
    corpus = os.path.join(out_dir, "corpus_sents.json")
    with open(corpus, "w") as f:
        json.dump(corpus_with_sents(a["docs"]), f)
    return corpus, a["raw_small"]


def case_argv(a, corpus, flags, save, index_path):
    return [a["raw_small"], "--indexpath", index_path, "--corpus_dict", corpus, "--retriever_path", a["ckpt"], "--reader_path",
            os.path.join(READER, "ckpt.pt"), "--save-prediction", save] + list(flags)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MDR_REFERENCE", "/root/reference"))
    ref_root = ap.parse_args().ref
    import warnings
    warnings.simplefilter("ignore")  # (a DataLoader pin_memory warning on a CPU-only host is not one of the script's log lines)
    import torch
    import transformers
    from oracle import gen_cli_golden as cli
    import gen_reader_golden as rg  # scripts/ (this file's directory) is sys.path[0] when run as a script

    tmp = tempfile.mkdtemp(prefix="mdr_e2e_golden_")
    a = cli.build_assets(tmp)
    corpus_path, _ = write_inputs(a, tmp)
    rcfg = transformers.AutoConfig.from_pretrained(READER)
    names = {"roberta-base": a["model_dir"], "google/electra-large-discriminator": READER}

    class FaissIndex:
        def __init__(self, xb):
            norms = (xb.astype(np.float64) ** 2).sum(1)
            self.xb = np.hstack([xb, np.sqrt(norms.max() - norms)[:, None].astype(np.float32)])  # the HNSW augmentation; queries add a 0 column

        def search(self, x, k):
            s = x @ self.xb.T
            I = np.argsort(-s, axis=1, kind="stable")[:, :k].astype(np.int64)
            D = -np.take_along_axis(s, I, axis=1).astype(np.float32)
            searches.append((D.copy(), I.copy()))
            return D, I

    meta, arrays, searches = {"cases": {}}, {}, []
    rg.install_stubs()
    cap = cli.Capture()
    sys.path[:0] = [ref_root, os.path.join(ref_root, "mdr")]
    for m in [m for m in sys.modules if m == "scripts" or m.startswith("scripts.")]:
        del sys.modules[m]
    with cli.stubbed(cap):
        sys.modules["faiss"].read_index = lambda path: FaissIndex(np.load(a["index"]))
        sys.modules["transformers"].AdamW = torch.optim.AdamW
        auto_tok = transformers.AutoTokenizer  # gen_cli_golden's 2.11 adapter for RoBERTa
        real_cfg, real_model = transformers.AutoConfig.from_pretrained, transformers.AutoModel.from_pretrained

        class AutoTokenizerE2E:
            @staticmethod
            def from_pretrained(name, *x, **k):
                return rg.Ref211Tokenizer(os.path.join(READER, "vocab.txt")) if "electra" in name else auto_tok.from_pretrained(names[name])

        def auto_model(name, *x, **k):
            if "electra" in name:
                return transformers.ElectraModel(rcfg)
            return transformers.RobertaModel(transformers.AutoConfig.from_pretrained(names[name]))

        transformers.AutoTokenizer = AutoTokenizerE2E
        transformers.AutoConfig.from_pretrained = staticmethod(lambda name, *x, **k: real_cfg(names.get(name, name)))
        transformers.AutoModel.from_pretrained = staticmethod(auto_model)
        import mdr.qa.qa_dataset as ref_ds
        import qa.qa_model as ref_qa_model
        sys.modules["transformers"].AdamW = torch.optim.AdamW  # (the lazy module object in sys.modules is replaced as models are imported)
        real_collate, real_forward = ref_ds.qa_collate, ref_qa_model.QAModel.forward
        try:
            for name, flags in CASES:
                batches, heads = [], []
                del searches[:]

                def collate(samples, pad_id=0):
                    b = real_collate(samples, pad_id=pad_id)
                    batches.append({"net": {k: v.numpy() for k, v in b["net_inputs"].items()}, "para_offsets": list(b["para_offsets"])})
                    return b

                def forward(self, batch):
                    o = real_forward(self, batch)
                    heads.append({k: v.detach().float().numpy() for k, v in o.items() if v is not None})
                    return o

                ref_ds.qa_collate = collate
                ref_qa_model.QAModel.forward = forward
                save = os.path.join(tmp, f"pred_{name}.json")
                out, err = io.StringIO(), io.StringIO()
                sys.argv = ["end2end.py"] + case_argv(a, corpus_path, flags, save, a["index"])
                sys.modules["transformers"].AutoTokenizer = AutoTokenizerE2E  # (set on the module object the script will import from)
                sys.modules["transformers"].AdamW = torch.optim.AdamW
                torch.manual_seed(0)
                with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
                    g = runpy.run_module("scripts.end2end", run_name="__main__", alter_sys=True)
                logging.getLogger().handlers.clear()
                id2doc = g["id2doc"]
                ident = {id(v): int(k) for k, v in id2doc.items()}
                chains = [[[ident[id(p[0])], ident[id(p[1])]] for p in r["candidate_chains"]] for r in g["retrieval_results"]]
                paths = []  # per question every (hop-1 id, hop-2 id, path score) of its k x k grid: the script's -(D + D') of the negated scores
                for (D1, I1), (D2, I2) in zip(searches[0::2], searches[1::2]):
                    k = I1.shape[1]
                    for b in range(I1.shape[0]):
                        paths.append([[int(I1[b, i]), int(I2[b * k + i, j]), float(-(D1[b, i] + D2[b * k + i, j]))] for i in range(k) for j in range(k)])
                meta["cases"][name] = {"flags": flags, "chains": chains, "paths": paths, "n_batches": len(batches),
                                       "para_offsets": [b["para_offsets"] for b in batches],
                                       "log": [ln for ln in err.getvalue().split("\n") if ln],
                                       "stdout": [("Finishing evaluation in <s>" if ln.startswith("Finishing evaluation in ") else ln)
                                                  for ln in out.getvalue().split("\n") if ln],
                                       "save_prediction": open(save).read()}
                for bi, (b, h) in enumerate(zip(batches, heads)):
                    for k, v in b["net"].items():
                        arrays[f"{name}.b{bi}.{k}"] = v
                    for k, v in h.items():
                        arrays[f"{name}.b{bi}.{k}"] = v
                sys.modules.pop("scripts.end2end", None)
        finally:
            ref_ds.qa_collate, ref_qa_model.QAModel.forward = real_collate, real_forward
            transformers.AutoConfig.from_pretrained, transformers.AutoModel.from_pretrained = real_cfg, real_model
            for p in (ref_root, os.path.join(ref_root, "mdr")):
                sys.path.remove(p)
    np.savez_compressed(os.path.join(GOLD, "end2end_ref.npz"), **arrays)
    with open(os.path.join(GOLD, "end2end_ref.json"), "w") as f:
        json.dump(meta, f)
    print({k: (len(v["chains"]), v["n_batches"], v["log"][-1]) for k, v in meta["cases"].items()})


if __name__ == "__main__":
    main()
