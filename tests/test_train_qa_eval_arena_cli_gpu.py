"""GPU (-m gpu): scripts/train_qa.py --eval-arena in child processes, each under a time limit of its own, against the same command without
the flag (the host path) on the committed tiny ELECTRA.

--do_predict with and without --sp-pred and --do_test: the same `__main__` log body and a byte-identical --save-prediction file; the
cache `<predict file>.qa_eval_pieces.npz` exists after the first run with the flag and the later ones log that they loaded it. A one-epoch
--do_train on the toy train file with its periodic and per-epoch evaluations: the same log body, checkpoint_last.pt byte for byte, and
checkpoint_best.pt likewise where the host path wrote one. A three-passage chain exits with the refusal and leaves no cache."""
import glob
import json
import os
import subprocess
import sys

import pytest

from test_train_qa_cli_gpu import load_script, main_lines, swap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")
SCRIPT = os.path.join(ROOT, "scripts", "train_qa.py")
PIECES_LINES = ("Loaded the reader's evaluation pieces from", "Preparing the dev set once for the reader as pieces")


def body(stderr):
    """The `__main__` log lines without the Namespace line (the flag and the output directory differ) and without the pieces' own lines."""
    return [ln for ln in main_lines(stderr) if not ln.startswith("Namespace(") and not ln.startswith(PIECES_LINES)]


def copy(src, dst):
    with open(dst, "wb") as f:
        f.write(open(src, "rb").read())
    return dst


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("qa_eval_cli"))
    model_dir = os.path.join(tmp, "electra-tiny")
    os.makedirs(model_dir)
    for n in ("config.json", "vocab.txt"):
        copy(os.path.join(ASSETS, n), os.path.join(model_dir, n))
    return {"tmp": tmp, "model_dir": model_dir, "dev": copy(os.path.join(ASSETS, "items.jsonl"), os.path.join(tmp, "dev.jsonl")),
            "train_host": copy(os.path.join(GOLD, "qa_train_items.jsonl"), os.path.join(tmp, "train_host.jsonl")),  # a copy per run: each builds
            "train_arena": copy(os.path.join(GOLD, "qa_train_items.jsonl"), os.path.join(tmp, "train_arena.jsonl")),  # its own training arena
            "train_dev": copy(os.path.join(GOLD, "qa_train_items.jsonl"), os.path.join(tmp, "train_dev.jsonl")),
            "ref": json.load(open(os.path.join(GOLD, "reader_ref.json")))}


def predict_run(s, mode, sp, flag, name):
    out = os.path.join(s["tmp"], name + ".json")
    cmd = [sys.executable, SCRIPT, mode, "--predict_file", s["dev"], "--init_checkpoint", os.path.join(ASSETS, "ckpt.pt"), "--model_name", s["model_dir"],
           "--fp16", "--max_ans_len", "35", "--max_seq_len", str(s["ref"]["max_seq_len"]), "--max_q_len", str(s["ref"]["max_q_len"]),
           "--predict_batch_size", str(s["ref"]["batch_size"]), "--num_workers", "0", "--save-prediction", out, "--output_dir", os.path.join(s["tmp"], "logs_" + name)]
    cmd += (["--sp-pred"] if sp else []) + (["--eval-arena"] if flag else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stderr, open(out, "rb").read()


# the three modes run in this order and share one predict file: the first run with the flag builds the cache, the later ones load it
@pytest.mark.parametrize("mode,sp", [("--do_predict", True), ("--do_predict", False), ("--do_test", True)], ids=["predict-sp", "predict-nosp", "test-sp"])
def test_flag_leaves_the_log_and_the_saved_prediction_alone(setup, mode, sp):
    cache = setup["dev"] + ".qa_eval_pieces.npz"
    had_cache = os.path.exists(cache)
    name = mode.strip("-") + ("_sp" if sp else "_nosp")
    host_err, host_bytes = predict_run(setup, mode, sp, False, name + "_host")
    assert os.path.exists(cache) == had_cache  # the host path neither reads nor writes it
    arena_err, arena_bytes = predict_run(setup, mode, sp, True, name + "_arena")
    assert body(arena_err) == body(host_err) and arena_bytes == host_bytes
    if mode == "--do_predict":
        assert any(ln.startswith("test performance {") for ln in body(host_err)) and len(body(host_err)) >= 13
        assert host_bytes == b"null" or set(json.loads(host_bytes)) == {"answer", "sp"}  # (best_res: null while the joint F1 stays 0)
    else:
        assert set(json.loads(host_bytes)) == {"answer", "sp", "titles"}
    assert os.path.exists(cache) and sorted(os.listdir(os.path.dirname(cache))).count("dev.jsonl.qa_eval_pieces.npz") == 1
    assert not glob.glob(cache + ".tmp*")
    said = [ln for ln in main_lines(arena_err) if ln.startswith(PIECES_LINES)]
    assert len(said) == 1 and said[0].startswith(PIECES_LINES[0] if had_cache else PIECES_LINES[1]), said
    if not had_cache:  # a second run with the flag logs a load and changes nothing
        again_err, again_bytes = predict_run(setup, mode, sp, True, name + "_again")
        assert [ln for ln in main_lines(again_err) if ln.startswith(PIECES_LINES)][0].startswith(PIECES_LINES[0])
        assert body(again_err) == body(host_err) and again_bytes == host_bytes


def train_run(s, gen, flag, name):
    out = os.path.join(s["tmp"], "train_" + name)
    argv = [sys.executable, SCRIPT] + gen.train_argv(s["model_dir"], os.path.join(ASSETS, "ckpt.pt"), out, extra=["--eval-arena"] if flag else [])
    for f, value in (("--train_file", s["train_" + name]), ("--predict_file", s["train_dev"]), ("--num_train_epochs", 1)):
        swap(argv, f, value)
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    (run,) = glob.glob(os.path.join(out, "*", "*"))
    return r.stderr, run


def test_training_evaluates_the_same_and_saves_the_same_checkpoints(setup):
    gen = load_script("gen_qa_train_golden")
    host_err, host_run = train_run(setup, gen, False, "host")
    arena_err, arena_run = train_run(setup, gen, True, "arena")
    lines = body(host_err)
    assert body(arena_err) == lines and lines[-1] == "Training finished!"
    assert sum(ln.startswith("evaluated ") for ln in lines) >= 2  # a periodic evaluation and the one after the epoch
    assert sum(ln.startswith(".......Using combination factor") for ln in lines) % 11 == 0
    assert sorted(os.listdir(arena_run)) == sorted(os.listdir(host_run)) and "checkpoint_last.pt" in os.listdir(host_run)
    for name in sorted(os.listdir(host_run)):
        if name.endswith(".pt"):
            assert open(os.path.join(arena_run, name), "rb").read() == open(os.path.join(host_run, name), "rb").read(), name
    assert os.path.exists(setup["train_dev"] + ".qa_eval_pieces.npz")


def test_a_three_passage_chain_exits_and_leaves_no_cache(setup):
    lines = [json.loads(ln) for ln in open(setup["dev"])]
    lines[1]["candidate_chains"][0] = lines[1]["candidate_chains"][0] + lines[1]["candidate_chains"][0][:1]
    bad = os.path.join(setup["tmp"], "three.jsonl")
    with open(bad, "w") as f:
        f.write("".join(json.dumps(x) + "\n" for x in lines))
    cmd = [sys.executable, SCRIPT, "--do_predict", "--eval-arena", "--predict_file", bad, "--init_checkpoint", os.path.join(ASSETS, "ckpt.pt"), "--model_name",
           setup["model_dir"], "--max_seq_len", "160", "--max_q_len", "24", "--predict_batch_size", "4", "--num_workers", "0", "--output_dir",
           os.path.join(setup["tmp"], "logs_three")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    last = r.stderr.strip().split("\n")[-1]
    assert last.startswith("--eval-arena is not supported: ") and "a chain of 3 passages" in last and "run without --eval-arena" in last
    assert not glob.glob(bad + ".*")
