"""CPU (-m "not gpu"): the host half of the reader on several ranks.

1  the batch deal of the evaluation (qa_eval.batch_deal): contiguous, disjoint runs in rank order that cover every batch, empty only when
   there are fewer batches than ranks
2  qa_eval.merge_tables on host tensors under dist.LoopbackWorld: every emulated rank ends with the table one rank fills, bit for bit, from
   local tables whose foreign rows and trailing sp_prob columns hold sentinels (-1, NaN patterns): nothing foreign is copied
3  dist.flat_layout(align=4): every offset a multiple of 4, the tensors in order and disjoint; align = 1 stays the running sum
4  scripts/train_qa.py: the four new flags parse to scripts/train_mhop.py's defaults, and every refusal of a launch exits non-zero with
   "training is not supported: " and its reason before any file is created; none says "multi-rank training is not built" any more
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny")
LAUNCH_KEYS = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


def load_script(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("n_batches", [0, 1, 2, 5, 79])
def test_the_batch_deal_is_contiguous_disjoint_and_complete(n_batches, N):
    from multihop_dense_retrieval_amd import qa_eval
    deal = qa_eval.batch_deal(n_batches, N)
    assert len(deal) == N and deal[0][0] == 0 and deal[-1][1] == n_batches
    assert all(deal[r][1] == deal[r + 1][0] for r in range(N - 1))  # contiguous and disjoint, in rank order
    assert [b for lo, hi in deal for b in range(lo, hi)] == list(range(n_batches))
    sizes = [hi - lo for lo, hi in deal]
    assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1
    assert (min(sizes) == 0) == (n_batches < N)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
N_ITEMS, MAX_SENTS = 23, 6


def head_of(lo, hi, s_b, sp):
    """decode()'s dict for rows lo .. hi - 1, every value naming its row: fp16 PATTERNS for the two scores (quiet and signalling NaNs, both
    infinities and negative zero among them: they travel as integers), positions up to 512, sp_prob on an fp16-exact grid."""
    rows = torch.arange(lo, hi)
    rank = ((rows * 2731 + 0x7C00) % 65536 - 32768).to(torch.int16)   # crosses the infinities and the NaN ranges of both signs
    span = ((rows * 1 + 0x7DFF) % 65536 - 32768).to(torch.int16)
    head = {"rank_score": rank.view(torch.float16).reshape(-1, 1), "span_score": span.view(torch.float16), "start": rows * 22 + 6, "end": 512 - rows}
    if sp:
        head["sp_prob"] = ((rows[:, None] * 8 + torch.arange(s_b)[None] + 1).float() / 256.0).to(torch.float16)
    return head


def cut(batch_size):
    batches = [(lo, min(N_ITEMS, lo + batch_size)) for lo in range(0, N_ITEMS, batch_size)]
    return batches, [(3 * b + 2) % (MAX_SENTS + 1) for b in range(len(batches))]  # S_b per batch: 2, 5, 1, 4, 0 for five batches


def bits(t):
    return None if t is None else t.contiguous().view(torch.uint8 if t.element_size() == 1 else {2: torch.int16, 8: torch.int64}[t.element_size()])


@pytest.mark.parametrize("sp", [True, False], ids=["sp", "nosp"])
@pytest.mark.parametrize("batch_size", [N_ITEMS, 5], ids=["1batch", "5batches"])
@pytest.mark.parametrize("N", [1, 2, 3, 8])
def test_the_merged_table_is_the_one_rank_table(N, batch_size, sp):
    from multihop_dense_retrieval_amd import dist, qa_eval
    batches, sents = cut(batch_size)
    assert len(batches) == {N_ITEMS: 1, 5: 5}[batch_size]
    want = qa_eval.ScoreTable(N_ITEMS, MAX_SENTS, "cpu")
    for (lo, hi), s_b in zip(batches, sents):
        want.put(lo, head_of(lo, hi, s_b, sp))

    def on_rank(w):
        local = qa_eval.ScoreTable(N_ITEMS, MAX_SENTS, "cpu")
        for t in (local.rank16, local.span16, local.start, local.end):
            t.fill_(-1)
        if sp:
            local.sp_prob = torch.full((N_ITEMS, MAX_SENTS), float("nan"), dtype=torch.float16)
        first, behind = qa_eval.batch_deal(len(batches), w.size)[w.rank]
        for (lo, hi), s_b in list(zip(batches, sents))[first:behind]:
            local.put(lo, head_of(lo, hi, s_b, sp))
        return qa_eval.merge_tables(local, batches, w)

    for r, got in enumerate(dist.LoopbackWorld(N).run(on_rank)):
        for name in ("rank16", "span16", "start", "end"):
            assert torch.equal(getattr(got, name), getattr(want, name)), (r, name)
        assert (got.sp_prob is None) == (want.sp_prob is None) == (not sp)
        if sp:
            assert torch.equal(bits(got.sp_prob), bits(want.sp_prob)), (r, "sp_prob")
        assert got.batch_lo == want.batch_lo == [lo for lo, _ in batches] and got.batch_sents == want.batch_sents, r
        assert [got.sents_of(i) for i in range(N_ITEMS)] == [want.sents_of(i) for i in range(N_ITEMS)]


def test_a_rank_that_filled_other_batches_is_refused():
    from multihop_dense_retrieval_amd import dist, qa_eval
    batches, sents = cut(5)

    def on_rank(w):
        local = qa_eval.ScoreTable(N_ITEMS, MAX_SENTS, "cpu")
        local.put(*[(lo, head_of(lo, hi, s, True)) for (lo, hi), s in zip(batches, sents)][0])  # every rank fills batch 0
        return qa_eval.merge_tables(local, batches, w)

    with pytest.raises(ValueError, match="decodes batches"):
        dist.LoopbackWorld(2).run(on_rank)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_flat_layout_aligns_the_readers_small_heads():
    from multihop_dense_retrieval_amd.dist import SEGMENT_MULTIPLE, flat_layout
    sizes = [64 * 30, 64, 2 * 64, 2, 64, 1, 64, 1]  # ..., qa_outputs.weight, qa_outputs.bias, rank.weight, rank.bias, sp.weight, sp.bias
    for N in (1, 2, 3, 16):
        offsets, S, padded = flat_layout(sizes, N, align=4)
        assert all(off % 4 == 0 for off in offsets) and offsets[0] == 0
        assert all(offsets[i] + sizes[i] <= offsets[i + 1] < offsets[i] + sizes[i] + 4 for i in range(len(sizes) - 1))
        assert S % SEGMENT_MULTIPLE == 0 and padded == N * S >= offsets[-1] + sizes[-1] > N * (S - SEGMENT_MULTIPLE) - N
        plain = flat_layout(sizes, N)
        assert plain == flat_layout(sizes, N, align=1) and plain[0] == [int(x) for x in np.cumsum([0] + sizes[:-1])]
        even = [64, 128, 4, 1]  # every size but the last a multiple of 4: the aligned layout has no gap (the retriever's case)
        assert flat_layout(even, N, align=4) == flat_layout(even, N)
    with pytest.raises(ValueError):
        flat_layout(sizes, 2, align=0)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_flags_parse_to_the_retrievers_defaults():
    from multihop_dense_retrieval_amd import config
    script = load_script("train_qa")
    d, m = script.train_args([]), config.train_args([])
    assert (d.dist_backend, d.share_gpu, d.dist_timeout, d.check_ranks, d.local_rank) == ("nccl", False, 1800, False, -1)
    assert (d.dist_backend, d.share_gpu, d.dist_timeout, d.check_ranks) == (m.dist_backend, m.share_gpu, m.dist_timeout, m.check_ranks)
    a = script.train_args("--dist-backend gloo --share-gpu --dist-timeout 120 --check-ranks".split())
    assert (a.dist_backend, a.share_gpu, a.dist_timeout, a.check_ranks) == ("gloo", True, 120, True)
    assert script.launch(d, environ={}) == (0, 1, -1)  # neither the flag nor a launcher: today's run
    env = {"RANK": "3", "LOCAL_RANK": "1", "WORLD_SIZE": "4", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "1"}
    assert script.launch(a, environ=env) == (3, 4, 1)
    with pytest.raises(SystemExit):
        script.train_args(["--dist-backend", "mpi"])


@pytest.fixture()
def model_dir(tmp_path):
    d = tmp_path / "electra-tiny"
    d.mkdir()
    for n in ("config.json", "vocab.txt"):
        (d / n).write_bytes(open(os.path.join(ASSETS, n), "rb").read())
    return str(d)


LAUNCHER = {"RANK": "1", "LOCAL_RANK": "1", "WORLD_SIZE": "2", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "1"}
REFUSALS = [  # (id, argv, the launcher's environment, what the message names)
    ("too-many-ranks", ["--dist-backend", "gloo", "--share-gpu"], dict(LAUNCHER, WORLD_SIZE="17"), ("17 ranks", "at most 16")),
    ("share-gpu-over-nccl", ["--share-gpu"], LAUNCHER, ("--share-gpu", "gloo only")),
    ("share-gpu-without-a-launcher", ["--share-gpu", "--dist-backend", "gloo"], {}, ("--share-gpu", "needs a launcher")),
    ("more-ranks-than-devices", ["--dist-backend", "gloo"], dict(LAUNCHER, RANK="15", LOCAL_RANK="15", WORLD_SIZE="16"), ("visible devices", "--share-gpu")),
    ("no-master-addr", ["--local_rank", "0"], {"WORLD_SIZE": "2"}, ("launcher", "MASTER_ADDR", "torchrun", "scripts/train_qa.py")),
]


@pytest.mark.parametrize("name,argv,env,said", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_of_a_launch_keeps_the_prefix(model_dir, tmp_path, name, argv, env, said):
    script = load_script("train_qa")
    args = script.train_args(["--do_train", "--model_name", model_dir, "--output_dir", str(tmp_path / "logs")] + argv)
    with pytest.raises(SystemExit) as e:
        script.check_train_inputs(args, environ=env)
    msg = e.value.code
    assert isinstance(msg, str) and msg.startswith("training is not supported: ") and all(s in msg for s in said), msg
    assert "multi-rank training is not built" not in msg and "train_mhop" not in msg
    assert not (tmp_path / "logs").exists()


@pytest.mark.parametrize("name", ["no-master-addr", "share-gpu-without-a-launcher"])
def test_the_command_line_exits_non_zero_before_any_file_is_created(model_dir, tmp_path, name):
    _, argv, env, said = next(r for r in REFUSALS if r[0] == name)
    full = {k: v for k, v in os.environ.items() if k not in LAUNCH_KEYS}
    full.update(env)
    before = sorted(os.listdir(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_qa.py"), "--do_train", "--model_name", model_dir, "--train_file",
                        os.path.join(ROOT, "tests", "golden", "qa_train_items.jsonl"), "--predict_file", os.path.join(ROOT, "tests", "golden", "qa_train_items.jsonl"),
                        "--output_dir", str(tmp_path / "logs")] + argv, capture_output=True, text=True, timeout=300, env=full)
    last = r.stderr.strip().split("\n")[-1]
    assert r.returncode != 0 and last.startswith("training is not supported: ") and all(s in last for s in said), r.stderr[-2000:]
    assert "multi-rank training is not built" not in r.stderr
    assert sorted(os.listdir(tmp_path)) == before and not os.path.exists(os.path.join(ROOT, "tests", "golden", "qa_train_items.jsonl.qa_train_arena.npz"))


def test_momentum_training_keeps_its_own_refusal():
    src = open(os.path.join(ROOT, "scripts", "train_momentum.py")).read()
    assert "multi-rank momentum training is not built" in src
