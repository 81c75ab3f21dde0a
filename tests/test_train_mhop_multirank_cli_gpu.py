"""GPU (-m gpu): scripts/train_mhop.py --do_train on two ranks, two child processes started here with RANK, WORLD_SIZE,
LOCAL_RANK, MASTER_ADDR and a free port, on the toy assets of tests/test_train_mhop_train_cli_gpu.py (2 epochs, batch 4, both dropout
probabilities 0.1).

The rehearsal: --dist-backend gloo --share-gpu --dist-timeout 120 --check-ranks, both ranks on device 0. Exit 0 twice; the reference's log
kinds from rank 0 alone, once; `ranks agree:` at every evaluation and at the end; both checkpoints with the reference's keys as finite fp32;
a second run under the same seed leaves the same bytes. With two visible devices the same command under nccl (RCCL), a device per rank, must
leave the gloo rehearsal's checkpoint_last.pt byte for byte: the gradient sum is this library's, so the transport cannot show in the bits.

Each child has a time limit; when one ends non-zero the other is stopped and nothing further is started."""
import glob
import importlib.util
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "train_mhop.py")
CHILD_SECONDS = 600
KINDS = ("Start training", "evaluated ", "MRR-1: ", "MRR-2: ", "Step ", "Saving model with best MRR", "Training finished!")


def load_script(name):
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main_lines(text):
    return [ln.split(" - __main__ - ", 1)[1] for ln in text.split("\n") if " - __main__ - " in ln]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def two_ranks(s, out, extra):
    """The training command on two ranks. Returns (rank 0's stderr, rank 1's stderr, the run directory)."""
    import time
    argv = [sys.executable, SCRIPT] + s["tgen"].train_argv(s["a"], s["train_file"], out, extra=extra)
    i = argv.index("--init_checkpoint")
    del argv[i:i + 2]
    port = free_port()
    os.makedirs(out, exist_ok=True)
    children, files = [], []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        files.append((open(os.path.join(out, f"rank{rank}.out"), "w+"), open(os.path.join(out, f"rank{rank}.err"), "w+")))
        children.append(subprocess.Popen(argv, stdout=files[rank][0], stderr=files[rank][1], env=env))
    deadline = time.monotonic() + CHILD_SECONDS
    try:
        while any(c.poll() is None for c in children):
            if time.monotonic() > deadline or any(c.poll() not in (None, 0) for c in children):
                break  # a rank failed or ran out of time: stop the other, start nothing further
            try:
                next(c for c in children if c.poll() is None).wait(timeout=1.0)
            except subprocess.TimeoutExpired:
                pass
    finally:
        for c in children:
            if c.poll() is None:
                c.kill()
                c.wait()
    texts = []
    for f_out, f_err in files:
        f_out.seek(0), f_err.seek(0)
        texts.append((f_out.read(), f_err.read()))
        f_out.close(), f_err.close()
    codes = [c.returncode for c in children]
    assert codes == [0, 0], (codes, texts[0][0][-1500:], texts[0][1][-3000:], texts[1][1][-3000:])
    runs = glob.glob(os.path.join(out, "*", "toy-seed*"))
    assert len(runs) == 1, runs
    return texts[0][1], texts[1][1], runs[0]


GLOO = ("--dist-backend", "gloo", "--share-gpu", "--dist-timeout", "120", "--check-ranks")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import transformers
    tmp = str(tmp_path_factory.mktemp("mhop_multirank_cli"))
    gen, tgen = load_script("gen_mhop_eval_golden"), load_script("gen_mhop_train_golden")
    a = gen.build_assets(tmp)
    hf = transformers.RobertaModel(transformers.AutoConfig.from_pretrained(a["model_dir"]))
    hf.load_state_dict({k[len("encoder."):]: torch.from_numpy(v) for k, v in a["sd"].items() if k.startswith("encoder.")}, strict=False)
    hf.save_pretrained(a["model_dir"])
    a["dev"] = os.path.join(tmp, "dev_bridge.jsonl")
    with open(a["dev"], "w") as f:
        f.write("\n".join(json.dumps(smp) for smp in a["samples"] if smp["type"] != "comparison"))
    train_file = os.path.join(tmp, "train.jsonl")
    tgen.write_train_file(train_file, tgen.train_samples())
    s = {"a": a, "tgen": tgen, "gen": gen, "train_file": train_file, "tmp": tmp,
         "meta": json.load(open(os.path.join(ROOT, "tests", "golden", "mhop_train_ref.json")))}
    s["err0"], s["err1"], s["run"] = two_ranks(s, os.path.join(tmp, "logs_gloo_a"), GLOO)
    return s


def test_two_ranks_on_one_card_log_once_agree_and_save_the_references_keys(setup):
    lines = main_lines(setup["err0"])
    assert main_lines(setup["err1"]) == [], "rank 1 wrote log lines"
    for kind in KINDS:
        assert any(ln.startswith(kind) for ln in lines), kind
    assert sum(ln.startswith("Start training") for ln in lines) == 1 and sum(ln == "Training finished!" for ln in lines) == 1
    assert any("distributed training True" in ln for ln in lines)
    evaluations = [i for i, ln in enumerate(lines) if ln.startswith("MRR-2: ")]
    agree = [i for i, ln in enumerate(lines) if ln.startswith("ranks agree: ")]
    assert len(evaluations) == 2 and len(agree) == 3 and agree[0] == evaluations[0] + 1 and agree[1] == evaluations[1] + 1, (evaluations, agree)
    assert all(len(lines[i].split(": ")[1]) == 16 and int(lines[i].split(": ")[1], 16) >= 0 for i in agree)
    assert lines[agree[0]] != lines[agree[1]] and lines[agree[1]] == lines[agree[2]]  # the parameters moved between the epochs, not behind the last
    steps = [ln for ln in lines if " MRR-AVG " in ln]
    assert len(steps) == 2 and steps[-1].startswith("Step 12 ")  # the full batch of 4 a step, whatever the rank count
    assert sorted(os.listdir(setup["run"])) == ["checkpoint_best.pt", "checkpoint_last.pt", "log.txt"]
    log = open(os.path.join(setup["run"], "log.txt")).read()
    assert log.count("Training finished!") == 1 and log.count("Start training") == 1
    want = sorted((k, tuple(shape)) for k, shape in setup["meta"]["checkpoint_last"])
    for name in ("checkpoint_best.pt", "checkpoint_last.pt"):
        sd = torch.load(os.path.join(setup["run"], name), map_location="cpu")
        assert sorted((k, tuple(v.shape)) for k, v in sd.items()) == want, name
        assert all(v.dtype == torch.float32 and not v.is_cuda and bool(torch.isfinite(v).all()) for v in sd.values())
    start = setup["a"]["sd"]
    last = torch.load(os.path.join(setup["run"], "checkpoint_last.pt"), map_location="cpu")
    assert not torch.equal(last["encoder.encoder.layer.0.output.dense.weight"], torch.from_numpy(start["encoder.encoder.layer.0.output.dense.weight"]))


def same_checkpoint(a_dir, b_dir, name):
    a, b = (torch.load(os.path.join(d, name), map_location="cpu") for d in (a_dir, b_dir))
    assert list(a) == list(b)
    for k in a:
        assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), (name, k)


def test_a_second_run_under_the_same_seed_leaves_the_same_bytes(setup):
    _, _, again = two_ranks(setup, os.path.join(setup["tmp"], "logs_gloo_b"), GLOO)
    for name in ("checkpoint_best.pt", "checkpoint_last.pt"):
        same_checkpoint(setup["run"], again, name)


def test_rccl_on_two_devices_leaves_the_gloo_rehearsals_bytes(setup):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (RCCL); one card runs the gloo rehearsal above, whose bytes this case compares with")
    err0, _, run = two_ranks(setup, os.path.join(setup["tmp"], "logs_nccl"), ("--dist-backend", "nccl", "--dist-timeout", "120", "--check-ranks"))
    assert sum(ln.startswith("ranks agree: ") for ln in main_lines(err0)) == 3
    same_checkpoint(setup["run"], run, "checkpoint_last.pt")
