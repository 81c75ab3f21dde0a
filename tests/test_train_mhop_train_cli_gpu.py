"""GPU (-m gpu): scripts/train_mhop.py --do_train end to end in child processes on the toy assets of scripts/gen_mhop_eval_golden.py: the toy
config as it is written (both dropout probabilities 0.1), the encoder's weights saved into the model directory (no --init_checkpoint:
project.* comes from torch's initialisers under --seed), the train file of scripts/gen_mhop_train_golden.py, 2 epochs, batch 4. The log is
held against the line formats of the reference's own run (tests/golden/mhop_train_ref.json), numbers free.

The dev file is the toy dev set WITHOUT its comparison questions. The reference shuffles a comparison question's two positives with the
global `random` generator on every read, at evaluation time too (multihop_dense_retrieval_amd/mhop_data.py), so such a question's rank in
the training run's last evaluation depends on every shuffle drawn before it; a fresh --do_predict process cannot be in that state, and the
comparison of its lines with the training run's, string for string, would compare two different dev sets. The comparison questions stay in
the train file."""
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
SCRIPT = os.path.join(ROOT, "scripts", "train_mhop.py")
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


def train_run(s, out, seed):
    argv = [sys.executable, SCRIPT] + s["tgen"].train_argv(s["a"], s["train_file"], out)
    argv[argv.index("--seed") + 1] = str(seed)
    i = argv.index("--init_checkpoint")
    del argv[i:i + 2]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    runs = glob.glob(os.path.join(out, "*", "*"))
    assert len(runs) == 1 and os.path.basename(runs[0]).startswith(f"toy-seed{seed}-bsz4-")
    return main_lines(r.stderr), runs[0]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import transformers
    tmp = str(tmp_path_factory.mktemp("mhop_train_cli"))
    gen, tgen = load_script("gen_mhop_eval_golden"), load_script("gen_mhop_train_golden")
    a = gen.build_assets(tmp)
    cfg = transformers.AutoConfig.from_pretrained(a["model_dir"])
    assert cfg.hidden_dropout_prob == 0.1 and cfg.attention_probs_dropout_prob == 0.1
    hf = transformers.RobertaModel(cfg)
    hf.load_state_dict({k[len("encoder."):]: torch.from_numpy(v) for k, v in a["sd"].items() if k.startswith("encoder.")}, strict=False)
    hf.save_pretrained(a["model_dir"])
    a["dev"] = os.path.join(tmp, "dev_bridge.jsonl")
    with open(a["dev"], "w") as f:
        f.write("\n".join(json.dumps(smp) for smp in a["samples"] if smp["type"] != "comparison"))
    train_file = os.path.join(tmp, "train.jsonl")
    tgen.write_train_file(train_file, tgen.train_samples())
    s = {"a": a, "tgen": tgen, "gen": gen, "train_file": train_file, "tmp": tmp,
         "meta": json.load(open(os.path.join(ROOT, "tests", "golden", "mhop_train_ref.json")))}
    s["lines"], s["run"] = train_run(s, os.path.join(tmp, "logs_a"), gen.SEED)
    return s


def pattern_of(line):
    return re.sub(r"\d+(?:\\\.\d+)?(?:e-?\d+)?", lambda m: NUM, re.escape(line))


def test_log_has_the_references_lines_and_both_checkpoints_its_keys(setup):
    ref = [ln.split(" - __main__ - ", 1)[1] for ln in setup["meta"]["log"]]
    kinds = ("Start training", "evaluated ", "MRR-1: ", "MRR-2: ", "Step ", "Saving model with best MRR", "Training finished!")
    lines = setup["lines"]
    for kind in kinds:
        pats = {pattern_of(ln) for ln in ref if ln.startswith(kind)}
        mine = [ln for ln in lines if ln.startswith(kind)]
        assert pats and mine, kind
        for ln in mine:
            assert any(re.fullmatch(p, ln) for p in pats), (kind, ln, pats)
    steps = [ln for ln in lines if " MRR-AVG " in ln]
    assert len(steps) == 2 and [ln.rsplit("=", 1)[1] for ln in steps] == ["0", "1"] and steps[-1].startswith("Step 12 ")
    assert lines[-1] == "Training finished!" and "Num of dev batches: 4" in lines
    assert sorted(os.listdir(setup["run"])) == ["checkpoint_best.pt", "checkpoint_last.pt", "log.txt"]
    assert "Training finished!" in open(os.path.join(setup["run"], "log.txt")).read()
    want = sorted((k, tuple(shape)) for k, shape in setup["meta"]["checkpoint_last"])
    for name in ("checkpoint_best.pt", "checkpoint_last.pt"):
        sd = torch.load(os.path.join(setup["run"], name), map_location="cpu")
        assert sorted((k, tuple(v.shape)) for k, v in sd.items()) == want, name
        assert all(v.dtype == torch.float32 and not v.is_cuda and bool(torch.isfinite(v).all()) for v in sd.values())
    start = setup["a"]["sd"]
    last = torch.load(os.path.join(setup["run"], "checkpoint_last.pt"), map_location="cpu")
    assert not torch.equal(last["encoder.encoder.layer.0.output.dense.weight"], torch.from_numpy(start["encoder.encoder.layer.0.output.dense.weight"]))
    assert torch.equal(last["encoder.pooler.dense.weight"], torch.from_numpy(start["encoder.pooler.dense.weight"]))  # carried, never stepped


def test_do_predict_reads_the_checkpoint_and_repeats_the_last_evaluation(setup):
    argv = [sys.executable, SCRIPT] + setup["gen"].cli_argv(setup["a"], [])
    argv[argv.index("--init_checkpoint") + 1] = os.path.join(setup["run"], "checkpoint_last.pt")
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    got = main_lines(r.stderr)
    last_eval = [ln for ln in setup["lines"] if ln.startswith(("evaluated ", "MRR-1: ", "MRR-2: "))][-3:]
    assert got[-4:-1] == last_eval
    assert got[-1].startswith("test performance {")
    mrr_avg = float(re.search(r"'mrr_avg': (?:np\.float64\()?([0-9.e-]+)", got[-1]).group(1))
    step = [ln for ln in setup["lines"] if " MRR-AVG " in ln][-1]
    assert f"MRR-AVG {mrr_avg * 100:.2f} " in step


def test_same_seed_same_bytes_other_seed_other_bytes(setup):
    seed = setup["gen"].SEED
    _, again = train_run(setup, os.path.join(setup["tmp"], "logs_b"), seed)
    _, other = train_run(setup, os.path.join(setup["tmp"], "logs_c"), seed + 1)
    for name in ("checkpoint_best.pt", "checkpoint_last.pt"):
        a, b = (torch.load(os.path.join(d, name), map_location="cpu") for d in (setup["run"], again))
        assert list(a) == list(b)
        for k in a:
            assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), (name, k, "two runs with one seed differ")
    a, c = (torch.load(os.path.join(d, "checkpoint_last.pt"), map_location="cpu") for d in (setup["run"], other))
    assert any(a[k].numpy().tobytes() != c[k].numpy().tobytes() for k in a if k.startswith("encoder.encoder."))
