"""Generate tests/golden/momentum_train_ref.{json,npz} by EXECUTING the reference's scripts/train_momentum.py --do_train --momentum (run
once, where the reference checkout is present):

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_momentum_train_golden.py [--ref /path/to/multihop_dense_retrieval]

The script runs as __main__ (runpy.run_path) on the CPU in fp32 with --num_workers 0, under the stubs, toy assets and train file of
scripts/gen_mhop_train_golden.py (both dropout probabilities 0; its TensorBoard stub and no-op pdb.set_trace included). Flags: batch 4,
--k 20, 2 epochs, --learning_rate 1e-4, no warmup, --eval-period -1, --init-retriever = the toy checkpoint. With --k 20 and 8 rows per step
the enqueue truncates at the end: 8, 8, then 4.

`.module` on one device: the reference reads model.module.queue (criterions.py) and model.module.encoder_q (its checkpoint lines), so on
one device, where it wraps nothing, it raises AttributeError. With torch.cuda.device_count patched to return 2 it wraps the model in
torch.nn.DataParallel, which on a CPU-only machine has no device ids and calls the module directly. That function is the one thing of
the run's behaviour that is patched. What the reference computed is captured by wrapping two of its own functions, as the mhop generator
does: mhop_collate (the collated tensors of every TRAIN batch) and mhop_loss (the queue before the first step, every batch's loss and
queue_ptr after every step), plus its __main__ log lines, the run directory's name and the checkpoint files' names and keys.

Only data is written: integers and floats. No weights and no program text.
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
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_mhop_eval_golden as base  # noqa: E402
import gen_mhop_train_golden as mhop  # noqa: E402

K, M, TEMPERATURE = 20, 0.999, 1


def momentum_argv(a, train_file, out_dir, k=K, extra=()):
    """The command line of the golden run (tests/test_train_momentum_cli_gpu.py runs the product with the same flags and its own --k)."""
    return ["--do_train", "--momentum", "--k", str(k), "--m", str(M), "--prefix", "toy", "--predict_batch_size", str(base.BATCH), "--train_batch_size",
            str(mhop.TRAIN_BATCH), "--model_name", a["model_dir"], "--train_file", train_file, "--predict_file", a["dev"], "--init-retriever", a["ckpt"],
            "--seed", str(base.SEED), "--max_c_len", str(base.MAX_C_LEN), "--max_q_len", str(base.MAX_Q_LEN), "--max_q_sp_len", str(base.MAX_Q_SP_LEN),
            "--num_workers", "0", "--num_train_epochs", str(mhop.EPOCHS), "--learning_rate", str(mhop.LR), "--warmup-ratio", "0", "--eval-period", "-1",
            "--output_dir", out_dir] + list(extra)


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
    script = os.path.join(ref_root, "scripts", "train_momentum.py")
    tmp = tempfile.mkdtemp(prefix="mdr_momentum_train_golden_")
    a = base.build_assets(tmp)
    mhop.zero_dropout(a["model_dir"])
    transformers.RobertaModel(transformers.AutoConfig.from_pretrained(a["model_dir"])).save_pretrained(a["model_dir"])
    samples = mhop.train_samples()
    ref_file = os.path.join(tmp, "train_ref.jsonl")
    mhop.write_train_file(ref_file, samples, for_reference=True)

    class Writer:
        def __init__(self, *x, **k):
            pass

        def add_scalar(self, *x, **k):
            pass

    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = Writer
    sys.modules["torch.utils.tensorboard"] = tb
    cli.RobertaTokenizer211.pad_token_id = property(lambda self: self.tok.pad_token_id)
    real_trace, pdb.set_trace = pdb.set_trace, lambda *x, **k: None  # (the dataset's train branch stops in one)

    batches, losses, ptrs, queue0, train_flags = [], [], [], [], []
    cap, err = cli.Capture(), io.StringIO()
    root_logger = logging.getLogger()
    root_logger.handlers.clear()
    out_dir = os.path.join(tmp, "logs")
    real_count = torch.cuda.device_count
    with cli.stubbed(cap), contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        sys.modules["transformers"].AdamW = torch.optim.AdamW
        import mdr.retrieval.criterions as ref_crit
        import mdr.retrieval.data.mhop_dataset as ref_ds
        real = (ref_ds.MhopDataset.__getitem__, ref_ds.mhop_collate, ref_crit.mhop_loss)

        def getitem(self, index):
            train_flags.append(bool(self.train))
            return real[0](self, index)

        def collate(samples_, pad_id=0):
            b = real[1](samples_, pad_id=pad_id)
            if train_flags[-1]:
                batches.append({k: v.numpy().copy() for k, v in b.items()})
            return b

        def mhop_loss(model, batch, args):
            if not queue0:
                queue0.append(model.module.queue.detach().numpy().copy())
            loss = real[2](model, batch, args)
            losses.append(float(loss.item()))
            ptrs.append(int(model.module.queue_ptr))
            return loss

        ref_ds.MhopDataset.__getitem__, ref_ds.mhop_collate, ref_crit.mhop_loss = getitem, collate, mhop_loss
        torch.cuda.device_count = lambda: 2  # the one patch of the run's behaviour: the reference then wraps its model (module docstring)
        try:
            sys.argv = [script] + momentum_argv(a, ref_file, out_dir)
            runpy.run_path(script, run_name="__main__")
        finally:
            torch.cuda.device_count = real_count
            ref_ds.MhopDataset.__getitem__, ref_ds.mhop_collate, ref_crit.mhop_loss = real
    pdb.set_trace = real_trace
    root_logger.handlers.clear()

    kept = len(samples) - 1  # the sample with a single tfidf negative is dropped
    n_batches = -(-kept // mhop.TRAIN_BATCH)
    assert len(batches) == len(losses) == len(ptrs) == mhop.EPOCHS * n_batches, (len(batches), len(losses), len(ptrs))
    sizes = [int(b["q_input_ids"].shape[0]) for b in batches]
    log = [ln for ln in err.getvalue().split("\n") if " - __main__ - " in ln and "Namespace(" not in ln]
    found = [os.path.join(dp, f) for dp, _, fs in os.walk(out_dir) for f in fs if f == "checkpoint_q_best.pt"]
    assert len(found) == 1, found
    run_dir = os.path.dirname(found[0])
    files = sorted(os.listdir(run_dir))
    ckpts = {f: torch.load(os.path.join(run_dir, f), map_location="cpu") for f in files if f.endswith(".pt")}
    meta = {"generator": "scripts/gen_momentum_train_golden.py: the reference's scripts/train_momentum.py --do_train --momentum executed as __main__ under "
                         "library stubs, torch.cuda.device_count patched to 2",
            "seed": base.SEED, "train_batch": mhop.TRAIN_BATCH, "epochs": mhop.EPOCHS, "learning_rate": mhop.LR, "k": K, "m": M, "temperature": TEMPERATURE,
            "max_q_len": base.MAX_Q_LEN, "max_q_sp_len": base.MAX_Q_SP_LEN, "max_c_len": base.MAX_C_LEN, "n_train_batches": len(batches),
            "batch_sizes": sizes, "queue_ptr": ptrs, "loss": losses, "log": [ln.replace(tmp, "<assets>") for ln in log],
            "run_dir": os.path.basename(run_dir), "files": files,
            "checkpoints": {f: [[k, list(v.shape)] for k, v in sd.items()] for f, sd in ckpts.items()},
            "checkpoint_dtypes": sorted({str(v.dtype) for sd in ckpts.values() for v in sd.values()})}
    arrays = {f"t{bi}.{k}": v.astype(np.int32) for bi, b in enumerate(batches) for k, v in b.items()}
    arrays["queue0"] = queue0[0].astype(np.float32)
    with open(os.path.join(GOLD, "momentum_train_ref.json"), "w") as f:
        json.dump(meta, f, indent=1)
    np.savez_compressed(os.path.join(GOLD, "momentum_train_ref.npz"), **arrays)
    print("\n".join(meta["log"]))
    print("loss", [round(x, 3) for x in losses])
    print("queue_ptr", ptrs, "batch sizes", sizes)
    print("run_dir", meta["run_dir"], "files", files)
    for n in ("momentum_train_ref.json", "momentum_train_ref.npz"):
        print(n, os.path.getsize(os.path.join(GOLD, n)), "bytes")


if __name__ == "__main__":
    main()
