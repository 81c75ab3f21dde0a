"""GPU (-m gpu): retriever training fed from the token arena (multihop_dense_retrieval_amd/mhop_arena.py, mdr_mhop_assemble) against the same
run fed the reference's way, on the toy assets of scripts/gen_mhop_eval_golden.py with the FULL toy dev set (comparison questions included,
as the train file's are): two epochs, --eval-period 2 so that evaluations interleave with the training reads, --gradient_accumulation_steps 2.

1  in process, scripts/train_mhop.py's train() under one seed with feed="arena" and with feed="host": the same checkpoint bytes, the same
   log lines, the same final states of `random` and of torch's generator; the same for scripts/train_momentum.py's step module
2  each script once in a child process: the reference's log lines only, exactly today's files in the run directory, the two caches beside
   the data files; a second run loads them, says so on stdout, and writes the same checkpoint bytes
"""
import glob
import importlib.util
import os
import random
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 24
EXTRA = ("--eval-period", "2", "--gradient_accumulation_steps", "2")


def load_script(name):
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    def __init__(self):
        self.lines = []

    def info(self, msg, *a):
        self.lines.append(msg % a if a else str(msg))


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    import transformers
    from multihop_dense_retrieval_amd import data
    tmp = str(tmp_path_factory.mktemp("mhop_feed"))
    gen, tgen, mgen = load_script("gen_mhop_eval_golden"), load_script("gen_mhop_train_golden"), load_script("gen_momentum_train_golden")
    a = gen.build_assets(tmp)
    train_file = os.path.join(tmp, "train.jsonl")
    tgen.write_train_file(train_file, tgen.train_samples())
    assert any(s["type"] == "comparison" for s in a["samples"]) and any(s["type"] == "comparison" for s in tgen.train_samples())
    cfg = transformers.AutoConfig.from_pretrained(a["model_dir"])
    assert cfg.hidden_dropout_prob == 0.1 and cfg.attention_probs_dropout_prob == 0.1  # dropout is live: the seeds must line up too
    return {"a": a, "gen": gen, "tgen": tgen, "mgen": mgen, "train_file": train_file, "tmp": tmp, "cfg": cfg, "tok": data.load_tokenizer(a["model_dir"]),
            "mhop": load_script("train_mhop"), "momentum": load_script("train_momentum")}


def run(env, feed, momentum):
    """The start-up of the script's main() (seeds, dev batches, model) and train() on `feed`, into a directory of its own."""
    from multihop_dense_retrieval_amd import mhop_data, momentum as momentum_steps, train as mdr_train
    from multihop_dense_retrieval_amd.config import train_args
    cli, mcli, a = env["mhop"], env["momentum"], env["a"]
    out = os.path.join(env["tmp"], f"{'momentum' if momentum else 'mhop'}_{feed}")
    os.makedirs(out)
    argv = env["mgen"].momentum_argv(a, env["train_file"], out, k=K, extra=EXTRA) if momentum else env["tgen"].train_argv(a, env["train_file"], out, extra=EXTRA)
    args = train_args(argv)
    args.train_batch_size = int(args.train_batch_size / args.accumulate_gradients)
    assert args.eval_period == 2 and args.gradient_accumulation_steps == 2 and args.num_train_epochs == 2 and args.output_dir == out
    device = torch.device("cuda", torch.cuda.current_device())
    collate_fc = partial(mhop_data.mhop_collate, pad_id=env["tok"].pad_token_id)
    log = Recorder()
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if momentum:
        args.momentum = True
        model = mcli.build_model(args, env["cfg"], device)
        dev = cli.dev_batches(args, env["tok"], collate_fc, device, feed=feed)
        log.info(f"Num of dev batches: {len(dev)}")
        cli.train(args, model, env["tok"], collate_fc, dev, device, log, None, steps=momentum_steps, eval_model=lambda: model,
                  saved=model.encoder_q.state_dict, best=mcli.CHECKPOINTS_BEST, last=mcli.CHECKPOINT_LAST, feed=feed)
    else:
        dev = cli.dev_batches(args, env["tok"], collate_fc, device, feed=feed)
        log.info(f"Num of dev batches: {len(dev)}")
        model = mdr_train.TrainableRetriever(env["cfg"], args)
        ckpt = torch.load(a["ckpt"], map_location="cpu")
        model.load_state_dict({k[7:]: v for k, v in ckpt.items() if k[7:] in model.shapes}, strict=False)
        model.to(device)
        cli.train(args, model, env["tok"], collate_fc, dev, device, log, None, feed=feed)
    torch.cuda.synchronize()
    files = {name: torch.load(os.path.join(out, name), map_location="cpu") for name in sorted(os.listdir(out))}
    return {"lines": log.lines, "random": random.getstate(), "torch": torch.get_rng_state(), "files": files}


def assert_same_run(arena, host, names):
    assert sorted(arena["files"]) == sorted(host["files"]) == sorted(names)
    for name in names:
        x, y = arena["files"][name], host["files"][name]
        assert list(x) == list(y)
        for k in x:
            assert x[k].dtype == y[k].dtype and x[k].numpy().tobytes() == y[k].numpy().tobytes(), (name, k, "the two feeds leave different bytes")
    assert arena["lines"] == host["lines"]
    assert arena["random"] == host["random"], "the two feeds leave `random` in different states"
    assert torch.equal(arena["torch"], host["torch"]), "the two feeds leave torch's generator in different states"
    lines = arena["lines"]
    assert lines[0] == "Num of dev batches: 6" and lines[-1] == "Training finished!"
    # 12 batches, boundaries at batch_step 1, 3, .. 11: 6 updates, an evaluation at updates 2, 4, 6 and one after each epoch
    assert sum(ln.startswith("Step ") and " MRR-AVG " not in ln for ln in lines) == 3 and sum(" MRR-AVG " in ln for ln in lines) == 2
    assert sum(ln.startswith("evaluated 24 examples") for ln in lines) == 5


def test_arena_feed_and_host_feed_leave_the_same_bytes(env):
    arena, host = run(env, "arena", False), run(env, "host", False)
    assert_same_run(arena, host, ["checkpoint_best.pt", "checkpoint_last.pt"])
    start = torch.load(env["a"]["ckpt"], map_location="cpu")
    name = "encoder.encoder.layer.0.output.dense.weight"
    assert not torch.equal(arena["files"]["checkpoint_last.pt"][name], start["module." + name]), "nothing was trained"


def test_momentum_arena_feed_and_host_feed_leave_the_same_bytes(env):
    arena, host = run(env, "arena", True), run(env, "host", True)
    assert_same_run(arena, host, ["checkpoint_k_best.pt", "checkpoint_q_best.pt", "checkpoint_q_last.pt"])
    start = torch.load(env["a"]["ckpt"], map_location="cpu")
    name = "encoder.encoder.layer.0.output.dense.weight"
    assert not torch.equal(arena["files"]["checkpoint_q_last.pt"][name], start["module." + name]), "encoder_q was not trained"


def test_unknown_feed_is_refused(env):
    from multihop_dense_retrieval_amd.config import train_args
    args = train_args(env["tgen"].train_argv(env["a"], env["train_file"], env["tmp"]))
    with pytest.raises(ValueError, match="feed"):
        env["mhop"].dev_batches(args, env["tok"], None, torch.device("cuda", 0), feed="workers")


def main_lines(stderr):
    return [ln.split(" - __main__ - ", 1)[1] for ln in stderr.split("\n") if " - __main__ - " in ln]


@pytest.mark.parametrize("script", ["train_mhop", "train_momentum"])
def test_cli_logs_the_references_lines_and_caches_beside_the_data(env, script, tmp_path):
    """Its own copies of the two data files, so that the caches it writes are this test's."""
    a = dict(env["a"], dev=str(tmp_path / "dev.jsonl"))
    train_file = str(tmp_path / "train.jsonl")
    for src, dst in ((env["a"]["dev"], a["dev"]), (env["train_file"], train_file)):
        with open(dst, "wb") as f:
            f.write(open(src, "rb").read())
    caches = [a["dev"] + ".mhop_arena.npz", train_file + ".mhop_arena.npz"]
    runs = []
    for attempt in ("first", "second"):
        out = str(tmp_path / f"logs_{attempt}")
        if script == "train_momentum":
            argv = env["mgen"].momentum_argv(a, train_file, out, k=K)
            want = ["checkpoint_k_best.pt", "checkpoint_q_best.pt", "checkpoint_q_last.pt", "log.txt"]
        else:
            argv = env["tgen"].train_argv(a, train_file, out)
            want = ["checkpoint_best.pt", "checkpoint_last.pt", "log.txt"]
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script + ".py")] + argv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        run_dir = glob.glob(os.path.join(out, "*", "*"))
        assert len(run_dir) == 1 and sorted(os.listdir(run_dir[0])) == want  # exactly the files of the run directory before the arena
        assert all(os.path.isfile(c) for c in caches) and sorted(os.listdir(tmp_path)) == sorted(
            ["dev.jsonl", "train.jsonl", "dev.jsonl.mhop_arena.npz", "train.jsonl.mhop_arena.npz"] + [f"logs_{x}" for x in ("first", "second")[:len(runs) + 1]])
        lines, log_txt = main_lines(r.stderr), open(os.path.join(run_dir[0], "log.txt")).read()
        kinds = ("Namespace(", "device ", "Num of dev batches: ", "TensorBoard is not installed", "Start training", "evaluated ", "MRR-1: ", "MRR-2: ", "Step ",
                 "Saving model with best MRR", "Training finished!")
        assert lines and all(ln.startswith(kinds) for ln in lines), [ln for ln in lines if not ln.startswith(kinds)]
        assert "Num of dev batches: 6" in lines and lines[-1] == "Training finished!"
        assert "arena" not in log_txt.split("Num of dev batches")[1].lower() and "Tokenising" not in log_txt and "Loaded the token arena" not in log_txt
        if attempt == "first":
            assert r.stdout.count("once into a token arena") == 2 and "Loaded the token arena" not in r.stdout
        else:
            assert r.stdout.count("Loaded the token arena") == 2 and "once into a token arena" not in r.stdout
            assert all(c in r.stdout for c in caches)
        runs.append({name: torch.load(os.path.join(run_dir[0], name), map_location="cpu") for name in want[:-1]})
    for name in runs[0]:
        for k in runs[0][name]:
            assert runs[0][name][k].numpy().tobytes() == runs[1][name][k].numpy().tobytes(), (name, k, "a run from the caches writes other bytes")
