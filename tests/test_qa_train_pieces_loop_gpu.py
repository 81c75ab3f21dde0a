"""GPU (-m gpu): scripts/train_qa.py --do_train fed from the piece arena (multihop_dense_retrieval_amd/qa_train_pieces.py,
mdr_reader_train_compose) against the same loop fed from the item arena (qa_train_arena.py, mdr_reader_train_assemble), on the committed
tiny ELECTRA (tests/golden/reader_electra_tiny) and the toy train file (tests/golden/qa_train_items.jsonl).

1  in process: two epochs of train() under one seed, dropout 0.1, leave byte-identical parameters and the same losses with either arena
   behind arena_batches;
2  through the command line, in child processes, each under a time limit of its own: --piece-arena writes a checkpoint_last.pt
   byte-identical to the run without it and logs the same lines; `<train file>.qa_train_pieces.npz` exists afterwards and a second run
   logs a load, not a build; a train file with a three-passage chain exits with "training is not supported: ...".
"""
import glob
import importlib.util
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import reader_train_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ITEMS = os.path.join(GOLD, "qa_train_items.jsonl")
SCRIPT = os.path.join(ROOT, "scripts", "train_qa.py")
CHILD_TIMEOUT = 300  # seconds, each child process


def load_script(name):
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Quiet:
    def __init__(self):
        self.lines = []

    def info(self, msg, *a):
        self.lines.append(msg % a if a else str(msg))


@pytest.fixture(scope="module")
def env():
    import transformers
    return {"cli": load_script("train_qa"), "gen": load_script("gen_qa_train_golden"), "meta": json.load(open(os.path.join(GOLD, "qa_train_ref.json"))),
            "tok": transformers.BertTokenizer(os.path.join(ref.ASSETS, "vocab.txt"), do_lower_case=True)}


def run(env, arena_class, dropout, extra=()):
    """scripts/train_qa.py's start-up (seeds, model, dataset, sampler, arena) and its train() with the golden run's flags; no evaluation, no
    files. Returns (train()'s result, the parameters as bytes, the index sequences the sampler drew)."""
    from multihop_dense_retrieval_amd import qa_train_data, reader_train
    cli, gen, tok = env["cli"], env["gen"], env["tok"]
    args = cli.train_args(gen.train_argv("electra-tiny", "", "", extra=("--eval-period", "-1") + tuple(extra)))
    assert args.sp_pred and args.output_dir == "" and args.seed == env["meta"]["seed"] and not args.piece_arena
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    model = reader_train.TrainableReader(ref.tiny_config(dropout, dropout), args)
    model.load_state_dict(ref.checkpoint(True))
    model.cuda()
    ds = qa_train_data.QATrainDataset(tok, ITEMS, args.max_seq_len, args.max_q_len)
    sampler = qa_train_data.MhopSampler(ds, num_neg=args.neg_num)
    drawn = []

    class Recording:
        def __len__(self):
            return len(sampler)

        def __iter__(self):
            drawn.append(list(iter(sampler)))
            return iter(drawn[-1])

    feed = cli.arena_batches(arena_class.from_dataset(ds).to("cuda"), tok.pad_token_id, torch.device("cuda", torch.cuda.current_device()))
    out = cli.train(args, model, Recording(), feed, lambda: {"em": 0.0}, Quiet())
    torch.cuda.synchronize()
    return out, {k: v.detach().cpu().numpy().tobytes() for k, v in model.state_dict().items()}, drawn


def test_piece_feed_and_item_feed_leave_the_same_bytes(env):
    from multihop_dense_retrieval_amd import qa_train_arena, qa_train_pieces
    p, pp, dp = run(env, qa_train_pieces.QATrainPieces, 0.1, ("--num_train_epochs", "2"))
    a, pa, da = run(env, qa_train_arena.QATrainArena, 0.1, ("--num_train_epochs", "2"))
    assert dp == da and len(dp) == 2 and p["global_step"] == a["global_step"] == 12
    assert p["loss"] == a["loss"] and len(p["loss"]) == 12
    assert list(pp) == list(pa)
    for k in pp:
        assert pp[k] == pa[k], (k, "the two arenas leave different parameters")
    start = ref.checkpoint(True)
    assert pp["encoder.encoder.layer.0.output.dense.weight"] != start["encoder.encoder.layer.0.output.dense.weight"].numpy().tobytes()


# ---- through the command line ---------------------------------------------------------------------------------------------------------------


def main_lines(stderr):
    return [ln.split(" - __main__ - ", 1)[1] for ln in stderr.split("\n") if " - __main__ - " in ln]


def cli_run(s, out, train_file, extra=()):
    argv = [sys.executable, SCRIPT] + s["gen"].train_argv(s["model_dir"], os.path.join(ref.ASSETS, "ckpt.pt"), out, extra=extra)
    for flag, value in (("--train_file", train_file), ("--predict_file", s["items"]), ("--num_train_epochs", 1), ("--eval-period", -1)):
        argv[argv.index(flag) + 1] = str(value)
    return subprocess.run(argv, capture_output=True, text=True, timeout=CHILD_TIMEOUT)


def finished(r, out):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    runs = glob.glob(os.path.join(out, "*", "*"))
    assert len(runs) == 1
    return main_lines(r.stderr), torch.load(os.path.join(runs[0], "checkpoint_last.pt"), map_location="cpu")


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("qa_train_pieces_cli"))
    model_dir = os.path.join(tmp, "electra-tiny")
    os.makedirs(model_dir)
    for n in ("config.json", "vocab.txt"):
        with open(os.path.join(model_dir, n), "wb") as f:
            f.write(open(os.path.join(ref.ASSETS, n), "rb").read())
    items = os.path.join(tmp, "items.jsonl")  # a copy: the caches are written beside the train file
    with open(items, "wb") as f:
        f.write(open(ITEMS, "rb").read())
    return {"gen": load_script("gen_qa_train_golden"), "model_dir": model_dir, "items": items, "tmp": tmp}


BODY = ("Namespace(", "Preparing", "Loaded", "Loading model from")  # the flags, the arena's own start-up line, a path: not compared


def body(lines):
    return [ln for ln in lines if not ln.startswith(BODY)]


def assert_same_weights(a, b, what):
    assert list(a) == list(b)
    for k in a:
        assert a[k].numpy().tobytes() == b[k].numpy().tobytes(), (k, what)


@pytest.fixture(scope="module")
def pair(setup):
    """The run without the flag, then the first run with it (which builds the pieces and writes the cache)."""
    s = setup
    cache = s["items"] + ".qa_train_pieces.npz"
    plain, ckpt_plain = finished(cli_run(s, os.path.join(s["tmp"], "logs_a"), s["items"]), os.path.join(s["tmp"], "logs_a"))
    assert not os.path.exists(cache) and os.path.exists(s["items"] + ".qa_train_arena.npz")
    first, ckpt_first = finished(cli_run(s, os.path.join(s["tmp"], "logs_b"), s["items"], extra=("--piece-arena",)), os.path.join(s["tmp"], "logs_b"))
    assert os.path.exists(cache)
    return {"plain": plain, "ckpt_plain": ckpt_plain, "first": first, "ckpt_first": ckpt_first}


def test_cli_with_the_piece_arena_writes_the_same_checkpoint_and_caches_the_pieces(pair):
    plain, first = pair["plain"], pair["first"]
    assert sum(ln.startswith("Preparing the training set once for the reader as pieces (29 items") for ln in first) == 1
    assert not any(ln.startswith("Loaded the reader's training pieces") for ln in first)
    assert not any("pieces" in ln for ln in plain if not ln.startswith("Namespace("))
    steps = [ln for ln in plain if ln.startswith("Step ")]
    assert len(steps) == 1 and steps[0].startswith("Step 6 Train loss ") and plain[-1] == "Training finished!"
    assert body(first) == body(plain)
    assert_same_weights(pair["ckpt_first"], pair["ckpt_plain"], "--piece-arena trains other weights")
    start = torch.load(os.path.join(ref.ASSETS, "ckpt.pt"), map_location="cpu")
    k = "encoder.encoder.layer.0.output.dense.weight"
    assert not torch.equal(pair["ckpt_plain"][k], start[k].float())


def test_cli_loads_the_cached_pieces_the_second_time(setup, pair):
    s = setup
    second, ckpt_second = finished(cli_run(s, os.path.join(s["tmp"], "logs_c"), s["items"], extra=("--piece-arena",)), os.path.join(s["tmp"], "logs_c"))
    assert sum(ln.startswith("Loaded the reader's training pieces") for ln in second) == 1 and not any(ln.startswith("Preparing") for ln in second)
    assert body(second) == body(pair["plain"])
    assert_same_weights(ckpt_second, pair["ckpt_plain"], "the loaded pieces train other weights")


def test_cli_names_the_default_arena_for_a_three_passage_chain(setup):
    s = setup
    lines = open(ITEMS).read().split("\n")
    rec = json.loads(lines[1])
    rec["candidate_chains"][0] = rec["candidate_chains"][0] + [rec["candidate_chains"][1][0]]
    train_file = os.path.join(s["tmp"], "three.jsonl")
    with open(train_file, "w") as f:
        f.write("\n".join([lines[0], json.dumps(rec)] + lines[2:]))
    r = cli_run(s, os.path.join(s["tmp"], "logs_three"), train_file, extra=("--piece-arena",))
    assert r.returncode != 0 and not os.path.exists(train_file + ".qa_train_pieces.npz")
    last = r.stderr.strip().split("\n")[-1]
    assert last.startswith("training is not supported: ") and "chain of 3 passages" in last and "default item arena" in last, r.stderr[-2000:]
