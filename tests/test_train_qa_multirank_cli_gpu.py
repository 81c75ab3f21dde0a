"""GPU (-m gpu): scripts/train_qa.py --do_train on two ranks, two child processes started here with RANK, WORLD_SIZE,
LOCAL_RANK, MASTER_ADDR and a free port, on the committed tiny ELECTRA (both dropout probabilities 0.1) and copies of the toy train file as
train and dev set: one epoch, batch 4, --eval-period 4, so a periodic evaluation and the one after the epoch.

The rehearsal: --dist-backend gloo --share-gpu --dist-timeout 120 --eval-arena --check-ranks, both ranks on device 0 (two processes with the
device open, far under the limit of 16). Exit 0 twice; rank 0 alone logs and writes log.txt and the checkpoints, nothing of rank 1 appears
under --output_dir; `ranks agree:` behind every evaluation and at the end; a second run leaves byte-identical checkpoint_last.pt and
checkpoint_best.pt; the evaluation blocks of the log whose weights were saved (the last one: checkpoint_last.pt; the last improvement:
checkpoint_best.pt) equal, line for line, qa_eval's one-rank evaluation of those weights with no world; --piece-arena leaves the item arena's
checkpoint bytes. With two visible devices the same command under nccl (RCCL), a device per rank, must leave the rehearsal's
checkpoint_last.pt byte for byte.

Each child has a time limit; when one ends non-zero the other is stopped and nothing further is started."""
import glob
import os
import subprocess
import sys
import time
import types

import pytest
import torch

from test_qa_eval_host import logged
from test_train_mhop_multirank_cli_gpu import free_port, main_lines, same_checkpoint
from test_train_qa_cli_gpu import load_script, swap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")
SCRIPT = os.path.join(ROOT, "scripts", "train_qa.py")
CHILD_SECONDS = 600
GLOO = ("--dist-backend", "gloo", "--share-gpu", "--dist-timeout", "120", "--eval-arena", "--check-ranks")


def copy(src, dst):
    with open(dst, "wb") as f:
        f.write(open(src, "rb").read())
    return dst


def two_ranks(s, name, extra):
    """The training command on two ranks. Returns (rank 0's stderr, rank 1's stderr, the run directory, --output_dir)."""
    out, side = os.path.join(s["tmp"], "logs_" + name), os.path.join(s["tmp"], "ranks_" + name)
    argv = [sys.executable, SCRIPT] + s["gen"].train_argv(s["model_dir"], os.path.join(ASSETS, "ckpt.pt"), out, extra=extra)
    for flag, value in (("--train_file", s["train"]), ("--predict_file", s["dev"]), ("--num_train_epochs", 1)):
        swap(argv, flag, value)
    port = free_port()
    os.makedirs(side)
    children, files = [], []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        files.append((open(os.path.join(side, f"rank{rank}.out"), "w+"), open(os.path.join(side, f"rank{rank}.err"), "w+")))
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
    return texts[0][1], texts[1][1], runs[0], out


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("qa_multirank_cli"))
    model_dir = os.path.join(tmp, "electra-tiny")
    os.makedirs(model_dir)
    for n in ("config.json", "vocab.txt"):
        copy(os.path.join(ASSETS, n), os.path.join(model_dir, n))
    s = {"gen": load_script("gen_qa_train_golden"), "model_dir": model_dir, "tmp": tmp,
         "train": copy(os.path.join(GOLD, "qa_train_items.jsonl"), os.path.join(tmp, "train.jsonl")),  # copies: the caches are written beside them
         "dev": copy(os.path.join(GOLD, "qa_train_items.jsonl"), os.path.join(tmp, "dev.jsonl"))}
    s["err0"], s["err1"], s["run"], s["out"] = two_ranks(s, "gloo_a", GLOO)
    return s


def blocks_of(lines):
    """[(index of `evaluated`, the lines from it to `Best joint F1`)] of a training log."""
    out = []
    for i, ln in enumerate(lines):
        if ln.startswith("evaluated "):
            j = next(k for k in range(i, len(lines)) if lines[k].startswith("Best joint F1"))
            out.append((i, lines[i:j + 1]))
    return out


def test_rank_zero_alone_logs_and_writes_and_the_ranks_agree(setup):
    lines = main_lines(setup["err0"])
    assert main_lines(setup["err1"]) == [], "rank 1 wrote log lines"
    assert any("distributed training True" in ln for ln in lines)
    assert sum(ln.startswith("Start training") for ln in lines) == 1 and lines[-1] == "Training finished!"
    assert not any("evaluates the whole dev set by the host path" in ln for ln in lines)  # --eval-arena: the batches are split
    blocks = blocks_of(lines)
    agree = [i for i, ln in enumerate(lines) if ln.startswith("ranks agree: ")]
    assert len(blocks) == 2 and len(agree) == 3, (len(blocks), agree)  # step 4, the epoch's end, and the end of the run
    for (i, block), a in zip(blocks, agree):
        assert a == i + len(block), "a `ranks agree:` line follows every evaluation block"
        assert len(block) == 3 + 7 * 11 and block[1].startswith("chain ranking em: ")
    assert all(len(lines[i].split(": ")[1]) == 16 and int(lines[i].split(": ")[1], 16) >= 0 for i in agree)
    assert lines[agree[0]] != lines[agree[1]] and lines[agree[1]] == lines[agree[2]]  # the parameters moved between the evaluations, not behind the last
    files = sorted(os.listdir(setup["run"]))
    assert files in (["checkpoint_best.pt", "checkpoint_last.pt", "log.txt"], ["checkpoint_last.pt", "log.txt"]), files
    assert ("checkpoint_best.pt" in files) == any(ln.startswith("Saving model with best em") for ln in lines)
    under = [os.path.relpath(os.path.join(d, f), setup["out"]) for d, _, fs in os.walk(setup["out"]) for f in fs]
    assert sorted(os.path.basename(f) for f in under) == files, under  # nothing of rank 1 under --output_dir
    log = open(os.path.join(setup["run"], "log.txt")).read()
    assert log.count("Training finished!") == 1 and log.count("Start training") == 1 and log.count("ranks agree: ") == 3
    start = torch.load(os.path.join(ASSETS, "ckpt.pt"), map_location="cpu")
    last = torch.load(os.path.join(setup["run"], "checkpoint_last.pt"), map_location="cpu")
    k = "encoder.encoder.layer.0.output.dense.weight"
    assert all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in last.values()) and not torch.equal(last[k], start[k].float())


def test_the_saved_weights_evaluate_on_one_rank_to_the_logs_blocks(setup):
    """The last block was logged on checkpoint_last.pt's weights, the block before the last `Saving model` line on checkpoint_best.pt's."""
    import transformers
    from multihop_dense_retrieval_amd import qa_eval, reader
    lines = main_lines(setup["err0"])
    blocks = blocks_of(lines)
    saved = {"checkpoint_last.pt": blocks[-1][1]}
    saving = [i for i, ln in enumerate(lines) if ln.startswith("Saving model with best em")]
    if saving:
        saved["checkpoint_best.pt"] = [b for i, b in blocks if i < saving[-1]][-1]
    tok = transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)
    cfg = transformers.AutoConfig.from_pretrained(ASSETS, local_files_only=True)
    meta = setup["gen"]
    pieces = qa_eval.QAEvalPieces.from_file(setup["dev"], tok, meta.MAX_SEQ_LEN, meta.MAX_Q_LEN, 8).to(torch.device("cuda", 0))
    for name, block in saved.items():
        model = reader.QAModel(cfg, types.SimpleNamespace(model_name="electra-tiny", sp_pred=True))
        reader.load_saved(model, os.path.join(setup["run"], name), exact=False, map_location="cpu")
        table = qa_eval.score_table(model.to("cuda").eval(), pieces, 35)
        _, want = logged("qa-multirank-cli-" + name, lambda lg: qa_eval.predict_metrics(pieces, table, tok, True, lg, fixed_thresh=None))
        assert block == want, name


def test_a_second_run_leaves_the_same_bytes(setup):
    _, _, again, _ = two_ranks(setup, "gloo_b", GLOO)
    for name in sorted(os.listdir(setup["run"])):
        if name.endswith(".pt"):
            same_checkpoint(setup["run"], again, name)
    assert sorted(os.listdir(again)) == sorted(os.listdir(setup["run"]))


def test_the_piece_arena_leaves_the_item_arenas_bytes_under_two_ranks(setup):
    err0, _, run, _ = two_ranks(setup, "gloo_pieces", GLOO + ("--piece-arena",))
    for name in sorted(os.listdir(setup["run"])):
        if name.endswith(".pt"):
            same_checkpoint(setup["run"], run, name)
    assert os.path.exists(setup["train"] + ".qa_train_pieces.npz")
    assert sum(ln.startswith("ranks agree: ") for ln in main_lines(err0)) == 3


def test_rccl_on_two_devices_leaves_the_gloo_rehearsals_bytes(setup):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (RCCL); one card runs the gloo rehearsal above, whose bytes this case compares with")
    err0, _, run, _ = two_ranks(setup, "nccl", ("--dist-backend", "nccl", "--dist-timeout", "120", "--eval-arena", "--check-ranks"))
    assert sum(ln.startswith("ranks agree: ") for ln in main_lines(err0)) == 3
    same_checkpoint(setup["run"], run, "checkpoint_last.pt")
