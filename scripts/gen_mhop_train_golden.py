"""Generate tests/golden/mhop_train_ref.{json,npz} by EXECUTING the reference's scripts/train_mhop.py --do_train (run once, where the
reference checkout is present):

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_mhop_train_golden.py [--ref /path/to/multihop_dense_retrieval]

The script runs as __main__ (runpy.run_path) on toy assets, on the CPU in fp32 with --num_workers 0, under the library stubs of
oracle/gen_cli_golden.py (apex / tqdm / cuda no-ops, the transformers-2.11 tokenizer adapter); on top of them a TensorBoard stub whose
writer accepts add_scalar, and a no-op pdb.set_trace (the reference's train branch stops in one). What the reference computed is captured
by wrapping three of its own functions:
    MhopDataset.__getitem__   the (dataset, index) sequence of every item, eval and train interleaved as the run reads them
    mhop_collate              the collated tensors of every TRAIN batch
    mhop_loss                 the loss of every train batch
plus its __main__ log lines and the keys and shapes of the checkpoint_last.pt it wrote.

Toy assets: gen_mhop_eval_golden.build_assets' model, checkpoint and 24 dev samples, and `train_samples()`: the same 24 samples as a train
file with three `tfidf_neg` passages on most of them (other titles and texts than `neg_paras`, so the replacement shows), ONE sample whose
`tfidf_neg` holds a single passage (the train branch drops it) and ONE sample without the key. The reference raises KeyError on a sample
without `tfidf_neg`; MhopTrainDataset keeps that sample's `neg_paras` (a documented deviation), so the file the REFERENCE reads carries that
sample's `neg_paras` under `tfidf_neg` as well -- the same data by the product's rule -- and the fixture keeps the sample without the key.
The toy config is rewritten with both dropout probabilities 0. Flags: batch 4, 2 epochs, --learning_rate 1e-4, no warmup, --eval-period -1.

The generator also asserts the learning condition of tests/test_train_step_gpu.py (case 6) on the reference's own model, loss and loop
body: the six committed dev batches of tests/golden/mhop_eval_ref.npz, two passes in order, torch Adam at a constant 1e-4 with the
reference's clip at 2.0, weight decay 0, dropout 0: every second-pass loss is at most half the same batch's first-pass loss. The twelve
losses are kept. Only data is written: integers and a few floats, no weights.
"""
import argparse
import contextlib
import copy
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
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_mhop_eval_golden as base  # noqa: E402

TRAIN_BATCH, EPOCHS, LR = 4, 2, 1e-4
DROPPED, KEYLESS = 7, 11  # the sample with a single tfidf negative; the sample without the key


def train_samples():
    out = copy.deepcopy(base.dev_samples())
    for i, s in enumerate(out):
        if i == KEYLESS:
            continue
        negs = s["neg_paras"]
        s["tfidf_neg"] = [{"title": f"Tfidf {i}.{n}", "text": negs[n % len(negs)]["text"] + f" tfidf {n}"} for n in range(1 if i == DROPPED else 3)]
    return out


def write_train_file(path, samples, for_reference=False):
    rows = copy.deepcopy(samples)
    if for_reference:
        rows[KEYLESS]["tfidf_neg"] = copy.deepcopy(rows[KEYLESS]["neg_paras"])
    with open(path, "w") as f:
        f.write("\n".join(json.dumps(s) for s in rows))


def zero_dropout(model_dir):
    path = os.path.join(model_dir, "config.json")
    cfg = json.load(open(path))
    cfg["hidden_dropout_prob"], cfg["attention_probs_dropout_prob"] = 0.0, 0.0
    json.dump(cfg, open(path, "w"), indent=1)


def train_argv(a, train_file, out_dir, extra=()):
    return ["--do_train", "--prefix", "toy", "--predict_batch_size", str(base.BATCH), "--train_batch_size", str(TRAIN_BATCH), "--model_name", a["model_dir"],
            "--train_file", train_file, "--predict_file", a["dev"], "--init_checkpoint", a["ckpt"], "--seed", str(base.SEED), "--max_c_len", str(base.MAX_C_LEN),
            "--max_q_len", str(base.MAX_Q_LEN), "--max_q_sp_len", str(base.MAX_Q_SP_LEN), "--shared-encoder", "--num_workers", "0", "--num_train_epochs", str(EPOCHS),
            "--learning_rate", str(LR), "--warmup-ratio", "0", "--eval-period", "-1", "--output_dir", out_dir] + list(extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MDR_REFERENCE", "/root/reference"))
    ref_root = ap.parse_args().ref
    import warnings
    warnings.simplefilter("ignore")
    import pdb
    import torch
    import transformers
    from oracle import gen_cli_golden as cli
    cli.REF = ref_root
    script = os.path.join(ref_root, "scripts", "train_mhop.py")
    tmp = tempfile.mkdtemp(prefix="mdr_mhop_train_golden_")
    a = base.build_assets(tmp)
    zero_dropout(a["model_dir"])
    transformers.RobertaModel(transformers.AutoConfig.from_pretrained(a["model_dir"])).save_pretrained(a["model_dir"])
    samples = train_samples()
    ref_file = os.path.join(tmp, "train_ref.jsonl")
    write_train_file(ref_file, samples, for_reference=True)

    class Writer:
        def __init__(self, *x, **k):
            pass

        def add_scalar(self, *x, **k):
            pass

    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = Writer
    sys.modules["torch.utils.tensorboard"] = tb
    cli.RobertaTokenizer211.pad_token_id = property(lambda self: self.tok.pad_token_id)
    real_trace, pdb.set_trace = pdb.set_trace, lambda *x, **k: None

    items, batches, losses, learning = [], [], [], [[], []]
    cap, err = cli.Capture(), io.StringIO()
    root_logger = logging.getLogger()
    root_logger.handlers.clear()
    out_dir = os.path.join(tmp, "logs")
    with cli.stubbed(cap), contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        sys.modules["transformers"].AdamW = torch.optim.AdamW
        import mdr.retrieval.criterions as ref_crit
        import mdr.retrieval.data.mhop_dataset as ref_ds
        import mdr.retrieval.models.mhop_retriever as ref_model
        import mdr.retrieval.utils.utils as ref_utils
        real = (ref_ds.MhopDataset.__getitem__, ref_ds.mhop_collate, ref_crit.mhop_loss)

        def getitem(self, index):
            items.append(["train" if self.train else "eval", int(index)])
            return real[0](self, index)

        def collate(samples_, pad_id=0):
            b = real[1](samples_, pad_id=pad_id)
            if items[-1][0] == "train":
                batches.append({k: v.numpy().copy() for k, v in b.items()})
            return b

        def mhop_loss(model, batch, args):
            loss = real[2](model, batch, args)
            losses.append(float(loss.item()))
            return loss

        ref_ds.MhopDataset.__getitem__, ref_ds.mhop_collate, ref_crit.mhop_loss = getitem, collate, mhop_loss
        try:
            sys.argv = [script] + train_argv(a, ref_file, out_dir)
            runpy.run_path(script, run_name="__main__")
        finally:
            ref_ds.MhopDataset.__getitem__, ref_ds.mhop_collate, ref_crit.mhop_loss = real
        # the learning condition of tests/test_train_step_gpu.py case 6, on the reference's model, loss and loop body
        z = np.load(os.path.join(GOLD, "mhop_eval_ref.npz"))
        dev_batches = [{k.split(".", 1)[1]: torch.from_numpy(z[k].astype(np.int64)) for k in z.files if k.startswith(f"b{bi}.") and ".emb." not in k}
                       for bi in range(6)]
        args = types.SimpleNamespace(model_name=a["model_dir"], momentum=False)
        model = ref_model.RobertaRetriever(transformers.AutoConfig.from_pretrained(a["model_dir"]), args)
        ref_utils.load_saved(model, a["ckpt"])
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=LR, eps=1e-8)
        for rnd in range(2):
            for b in dev_batches:
                loss = real[2](model, b, args)
                loss.backward()
                learning[rnd].append(float(loss.item()))
                torch.nn.utils.clip_grad_norm_(model.parameters(), 2.0)
                opt.step()
                model.zero_grad()
    pdb.set_trace = real_trace
    root_logger.handlers.clear()
    for first, second in zip(*learning):
        assert second <= 0.5 * first, ("the learning condition fails on the reference itself", learning)

    kept = [s for i, s in enumerate(samples) if i != DROPPED]
    n_batches = -(-len(kept) // TRAIN_BATCH)
    assert len(batches) == len(losses) == EPOCHS * n_batches, (len(batches), len(losses))
    train_idx = [i for tag, i in items if tag == "train"]
    assert len(train_idx) == EPOCHS * len(kept) and sorted(set(train_idx)) == list(range(len(kept)))
    log = [ln for ln in err.getvalue().split("\n") if " - __main__ - " in ln and "Namespace(" not in ln]
    run_dir = [os.path.join(dp, f) for dp, _, fs in os.walk(out_dir) for f in fs if f == "checkpoint_last.pt"]
    assert len(run_dir) == 1 and os.path.exists(os.path.join(os.path.dirname(run_dir[0]), "checkpoint_best.pt")) \
        and os.path.exists(os.path.join(os.path.dirname(run_dir[0]), "log.txt"))
    ckpt = torch.load(run_dir[0], map_location="cpu")
    meta = {"generator": "scripts/gen_mhop_train_golden.py: the reference's scripts/train_mhop.py --do_train executed as __main__ under library stubs",
            "seed": base.SEED, "train_batch": TRAIN_BATCH, "epochs": EPOCHS, "learning_rate": LR, "max_q_len": base.MAX_Q_LEN,
            "max_q_sp_len": base.MAX_Q_SP_LEN, "max_c_len": base.MAX_C_LEN, "dropped": DROPPED, "keyless": KEYLESS, "n_train_batches": len(batches),
            "samples": samples, "items": items, "loss": losses, "log": [ln.replace(tmp, "<assets>") for ln in log],
            "run_dir": os.path.relpath(os.path.dirname(run_dir[0]), out_dir).split(os.sep)[-1],
            "checkpoint_last": [[k, list(v.shape)] for k, v in ckpt.items()], "checkpoint_dtypes": sorted({str(v.dtype) for v in ckpt.values()}),
            "learning_losses": learning}
    arrays = {f"t{bi}.{k}": v.astype(np.int32) for bi, b in enumerate(batches) for k, v in b.items()}
    with open(os.path.join(GOLD, "mhop_train_ref.json"), "w") as f:
        json.dump(meta, f, indent=1)
    np.savez_compressed(os.path.join(GOLD, "mhop_train_ref.npz"), **arrays)
    print("\n".join(meta["log"]))
    print("loss", [round(x, 3) for x in losses])
    print("learning", [[round(x, 2) for x in row] for row in learning])
    for n in ("mhop_train_ref.json", "mhop_train_ref.npz"):
        print(n, os.path.getsize(os.path.join(GOLD, n)), "bytes")


if __name__ == "__main__":
    main()
