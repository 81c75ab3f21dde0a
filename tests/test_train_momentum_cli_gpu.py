"""GPU (-m gpu): scripts/train_momentum.py end to end in child processes on the toy assets of scripts/gen_mhop_eval_golden.py: the toy config
as it is written (both dropout probabilities 0.1, so the key encoder's training-mode forward is live), the encoder's weights saved into the
model directory and the toy checkpoint as --init-retriever, the train file of scripts/gen_mhop_train_golden.py, batch 4, --k 24, 2 epochs.
The log is held against the line formats of the reference's own run (tests/golden/momentum_train_ref.json), numbers free. The dev file is
the toy dev set without its comparison questions, for the reason tests/test_train_mhop_train_cli_gpu.py gives."""
import glob
import json
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "train_momentum.py")
K = 24
FILES = ["checkpoint_k_best.pt", "checkpoint_q_best.pt", "checkpoint_q_last.pt", "log.txt"]
NUM = r"[-+0-9.e]+"


def load_script(name):
    import importlib.util
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main_lines(stderr):
    return [ln.split(" - __main__ - ", 1)[1] for ln in stderr.split("\n") if " - __main__ - " in ln]


def pattern_of(line):
    return re.sub(r"\d+(?:\\\.\d+)?(?:e-?\d+)?", lambda m: NUM, re.escape(line))


def train_run(s, out, seed):
    argv = [sys.executable, SCRIPT] + s["mgen"].momentum_argv(s["a"], s["train_file"], out, k=K)
    argv[argv.index("--seed") + 1] = str(seed)
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    runs = glob.glob(os.path.join(out, "*", "*"))
    assert len(runs) == 1 and os.path.basename(runs[0]).startswith(f"toy-seed{seed}-bsz4-") and os.path.basename(runs[0]).endswith(f"-m0.999-k{K}-t1")
    return main_lines(r.stderr), runs[0]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import transformers
    tmp = str(tmp_path_factory.mktemp("momentum_cli"))
    gen, tgen, mgen = load_script("gen_mhop_eval_golden"), load_script("gen_mhop_train_golden"), load_script("gen_momentum_train_golden")
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
    s = {"a": a, "gen": gen, "mgen": mgen, "train_file": train_file, "tmp": tmp,
         "meta": json.load(open(os.path.join(ROOT, "tests", "golden", "momentum_train_ref.json")))}
    s["lines"], s["run"] = train_run(s, os.path.join(tmp, "logs_a"), gen.SEED)
    return s


def test_log_has_the_references_lines_and_the_checkpoints_its_keys(setup):
    ref = [ln.split(" - __main__ - ", 1)[1] for ln in setup["meta"]["log"]]
    lines = setup["lines"]
    for kind in ("Start training", "evaluated ", "MRR-1: ", "MRR-2: ", "Step ", "Saving model with best MRR", "Training finished!"):
        pats = {pattern_of(ln) for ln in ref if ln.startswith(kind)}
        mine = [ln for ln in lines if ln.startswith(kind)]
        assert pats and mine, kind
        for ln in mine:
            assert any(re.fullmatch(p, ln) for p in pats), (kind, ln, pats)
    steps = [ln for ln in lines if " MRR-AVG " in ln]
    assert len(steps) == 2 and [ln.rsplit("=", 1)[1] for ln in steps] == ["0", "1"] and steps[-1].startswith("Step 12 ")
    assert lines[-1] == "Training finished!" and "Num of dev batches: 4" in lines
    assert sorted(os.listdir(setup["run"])) == FILES
    assert "Training finished!" in open(os.path.join(setup["run"], "log.txt")).read()
    want = sorted((k, tuple(shape)) for k, shape in setup["meta"]["checkpoints"]["checkpoint_q_best.pt"] if not k.endswith("position_ids"))
    sds = {name: torch.load(os.path.join(setup["run"], name), map_location="cpu") for name in FILES[:3]}
    for name, sd in sds.items():
        assert sorted((k, tuple(v.shape)) for k, v in sd.items()) == want, name
        assert all(v.dtype == torch.float32 and not v.is_cuda and bool(torch.isfinite(v).all()) for v in sd.values())
    q, k = sds["checkpoint_q_best.pt"], sds["checkpoint_k_best.pt"]
    assert all(torch.equal(q[n], k[n]) for n in q)  # the reference saves encoder_q twice
    start = setup["a"]["sd"]
    name = "encoder.encoder.layer.0.output.dense.weight"
    assert not torch.equal(sds["checkpoint_q_last.pt"][name], torch.from_numpy(start[name])), "encoder_q was not trained"


def test_do_predict_of_both_scripts_prints_the_same_lines(setup):
    """With the key encoder copied from the loaded weights, train_momentum.py --do_predict --init-retriever and train_mhop.py --do_predict
    --init_checkpoint are the same computation."""
    ckpt = os.path.join(setup["run"], "checkpoint_q_last.pt")
    base = setup["gen"].cli_argv(setup["a"], [])
    i = base.index("--init_checkpoint")
    mhop = [sys.executable, os.path.join(ROOT, "scripts", "train_mhop.py")] + base[:i] + ["--init_checkpoint", ckpt] + base[i + 2:]
    mom = [sys.executable, SCRIPT] + base[:i] + ["--init-retriever", ckpt, "--k", str(K)] + base[i + 2:]
    got = []
    for argv in (mhop, mom):
        r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = main_lines(r.stderr)
        assert lines[-1].startswith("test performance {")
        got.append([ln for ln in lines if ln.startswith(("evaluated ", "MRR-1: ", "MRR-2: "))])
    assert len(got[0]) == 3 and got[0] == got[1], got


def test_same_seed_same_bytes_other_seed_other_bytes(setup):
    seed = setup["gen"].SEED
    _, again = train_run(setup, os.path.join(setup["tmp"], "logs_b"), seed)
    _, other = train_run(setup, os.path.join(setup["tmp"], "logs_c"), seed + 1)
    for name in FILES[:3]:
        a, b = (torch.load(os.path.join(d, name), map_location="cpu") for d in (setup["run"], again))
        assert list(a) == list(b)
        for k in a:
            assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), (name, k, "two runs with one seed differ")
    a, c = (torch.load(os.path.join(d, "checkpoint_q_last.pt"), map_location="cpu") for d in (setup["run"], other))
    assert any(a[k].numpy().tobytes() != c[k].numpy().tobytes() for k in a if k.startswith("encoder.encoder."))


def test_train_mhop_still_refuses_momentum(setup):
    argv = [sys.executable, os.path.join(ROOT, "scripts", "train_mhop.py")] + setup["mgen"].momentum_argv(setup["a"], setup["train_file"],
                                                                                                         os.path.join(setup["tmp"], "logs_refused"), k=K)
    r = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--momentum is not built" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(os.path.join(setup["tmp"], "logs_refused"))
