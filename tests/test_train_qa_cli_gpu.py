"""GPU (-m gpu): scripts/train_qa.py --do_train end to end in child processes on the committed tiny ELECTRA (config as committed: both
dropout probabilities 0.1; weights from --init_checkpoint reader_electra_tiny/ckpt.pt) and a copy of the toy train file
(tests/golden/qa_train_items.jsonl) as train and dev set, 2 epochs, batch 4, --eval-period 4. The log is held against the line formats of
the reference's own run (tests/golden/qa_train_ref.json), numbers free. This is the test that fails before --do_train exists: the script
exits before it runs."""
import glob
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")
SCRIPT = os.path.join(ROOT, "scripts", "train_qa.py")
NUM = r"[-+0-9.e]+"


def load_script(name):
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main_lines(stderr):
    return [ln.split(" - __main__ - ", 1)[1] for ln in stderr.split("\n") if " - __main__ - " in ln]


def swap(argv, flag, value):
    argv[argv.index(flag) + 1] = str(value)


def train_run(s, out, seed):
    argv = [sys.executable, SCRIPT] + s["gen"].train_argv(s["model_dir"], os.path.join(ASSETS, "ckpt.pt"), out)
    for flag, value in (("--seed", seed), ("--train_file", s["items"]), ("--predict_file", s["items"]), ("--num_train_epochs", 2)):
        swap(argv, flag, value)
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    runs = glob.glob(os.path.join(out, "*", "*"))
    assert len(runs) == 1 and os.path.basename(runs[0]).startswith(f"toy-seed{seed}-bsz4-")
    return main_lines(r.stderr), runs[0]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("qa_train_cli"))
    model_dir = os.path.join(tmp, "electra-tiny")
    os.makedirs(model_dir)
    for n in ("config.json", "vocab.txt"):
        with open(os.path.join(model_dir, n), "wb") as f:
            f.write(open(os.path.join(ASSETS, n), "rb").read())
    items = os.path.join(tmp, "items.jsonl")  # a copy: the arena cache is written beside the train file
    with open(items, "wb") as f:
        f.write(open(os.path.join(GOLD, "qa_train_items.jsonl"), "rb").read())
    s = {"gen": load_script("gen_qa_train_golden"), "model_dir": model_dir, "items": items, "tmp": tmp,
         "meta": json.load(open(os.path.join(GOLD, "qa_train_ref.json")))}
    s["lines"], s["run"] = train_run(s, os.path.join(tmp, "logs_a"), s["meta"]["seed"])
    return s


def pattern_of(line):
    return re.sub(r"\d+(?:\\\.\d+)?(?:e-?\d+)?", lambda m: NUM, re.escape(line))


def test_log_has_the_references_lines_and_the_checkpoints_its_keys(setup):
    from multihop_dense_retrieval_amd import reader
    import reader_train_ref as ref
    golden = setup["meta"]["train"]
    kinds = ("device ", "Num of dev batches", "Loading model from", "Start training", "evaluated ", "chain ranking em: ", ".......Using combination factor",
             "answer em: ", "answer f1: ", "sp em: ", "sp f1: ", "joint em: ", "joint f1: ", "Best joint F1", "Step ", "Training finished!")
    lines = setup["lines"]
    for kind in kinds:
        pats = {pattern_of(ln) for ln in golden["log"] if ln.startswith(kind)}
        mine = [ln for ln in lines if ln.startswith(kind)]
        assert pats and mine, kind
        if kind in ("device ", "Loading model from"):
            continue  # (a path and a device name: present, not compared)
        for ln in mine:
            assert any(re.fullmatch(p, ln) for p in pats), (kind, ln, pats)
    saving = [ln for ln in lines if ln.startswith("Saving model with best em")]
    pats = {pattern_of(ln) for ln in golden["log"] if ln.startswith("Saving model with best em")}
    assert all(any(re.fullmatch(p, ln) for p in pats) for ln in saving)
    steps = [ln for ln in lines if ln.startswith("Step ")]
    assert [ln for ln in steps if " on epoch=" not in ln][-1].startswith("Step 12 ") and sum(" on epoch=" in ln for ln in steps) == 3  # steps 4, 8, 12
    assert lines[-1] == "Training finished!" and "Num of dev batches: 4" in lines
    assert len([ln for ln in lines if ln.startswith(".......Using combination factor")]) == 11 * 5  # the sweep, at 3 periods and 2 epochs
    want_files = ["checkpoint_last.pt", "log.txt"] + (["checkpoint_best.pt"] if saving else [])
    assert sorted(os.listdir(setup["run"])) == sorted(want_files)
    assert "Training finished!" in open(os.path.join(setup["run"], "log.txt")).read()
    want = sorted((k, tuple(shape)) for k, shape in reader.expected_state_dict_shapes(ref.tiny_config(), "electra", True).items())
    assert want == sorted((k, tuple(shape)) for k, shape in golden["state_dict"])  # the reference model's own parameters
    for name in want_files[:1] + want_files[2:]:
        sd = torch.load(os.path.join(setup["run"], name), map_location="cpu")
        assert sorted((k, tuple(v.shape)) for k, v in sd.items()) == want, name
        assert all(v.dtype == torch.float32 and not v.is_cuda and bool(torch.isfinite(v).all()) for v in sd.values())
    start = torch.load(os.path.join(ASSETS, "ckpt.pt"), map_location="cpu")
    last = torch.load(os.path.join(setup["run"], "checkpoint_last.pt"), map_location="cpu")
    k = "encoder.encoder.layer.0.output.dense.weight"
    assert not torch.equal(last[k], start[k].float()) and not torch.equal(last["pooler.dense.weight"], start["pooler.dense.weight"].float())


def test_do_predict_reads_the_checkpoint_and_repeats_the_last_evaluation(setup):
    argv = [sys.executable, SCRIPT, "--do_predict", "--model_name", setup["model_dir"], "--predict_file", setup["items"], "--init_checkpoint",
            os.path.join(setup["run"], "checkpoint_last.pt"), "--max_seq_len", str(setup["meta"]["max_seq_len"]), "--max_q_len", str(setup["meta"]["max_q_len"]),
            "--predict_batch_size", "8", "--sp-pred", "--output_dir", os.path.join(setup["tmp"], "logs_p")]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    got = main_lines(r.stderr)
    lines = setup["lines"]
    last = max(i for i, ln in enumerate(lines) if ln.startswith("evaluated "))
    at = lines.index(".......Using combination factor 0.8......", last)
    want = lines[last:last + 2] + lines[at:at + 7]  # evaluated, chain ranking em; the factor-0.8 block of the sweep
    first = got.index(want[0])
    assert got[first:first + 9] == want
    assert got[-1].startswith("test performance {")


def test_same_seed_same_bytes_other_seed_other_bytes(setup):
    seed = setup["meta"]["seed"]
    _, again = train_run(setup, os.path.join(setup["tmp"], "logs_b"), seed)
    _, other = train_run(setup, os.path.join(setup["tmp"], "logs_c"), seed + 1)
    a, b, c = (torch.load(os.path.join(d, "checkpoint_last.pt"), map_location="cpu") for d in (setup["run"], again, other))
    assert list(a) == list(b)
    for k in a:
        assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), (k, "two runs with one seed differ")
    assert any(a[k].numpy().tobytes() != c[k].numpy().tobytes() for k in a if k.startswith("encoder.encoder."))
