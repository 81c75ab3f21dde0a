"""GPU (-m gpu): the loop of scripts/train_qa.py --do_train, in process, on the committed tiny ELECTRA (tests/golden/reader_electra_tiny)
and the toy train file (tests/golden/qa_train_items.jsonl), against the reference's own run of its script (tests/golden/qa_train_ref.json,
"train": CPU, fp32, dropout 0, from reader_electra_tiny/ckpt.pt).

1  two epochs fed from the arena (mdr_reader_train_assemble) and two epochs fed from the host path (__getitem__, qa_train_collate, upload)
   under one seed, dropout 0.1, leave byte-identical parameters -- and the same losses
2  dropout 0, the golden's flags: the sampler draws the reference run's index sequences; the first batch's loss against the reference's
   first recorded loss, asserted at FIRST_LOSS_REL; the epoch means fall from the first epoch to the last, as the golden's do
3  --gradient_accumulation_steps 2: the optimizer steps are the reference's boundary count, (batch_step + 1) % 2 == 0
"""
import importlib.util
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

import reader_train_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ITEMS = os.path.join(GOLD, "qa_train_items.jsonl")
# |loss - reference| / reference of the first batch: 4 x the error measured on an MI355X (profiles/qa_train_loop.md), rounded up to a power
# of two. The reference is fp32 on the CPU; the product's trunk computes in fp16.
FIRST_LOSS_REL = 2.0 ** -11  # measured 6.9e-5 = 2^-13.8


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
    meta = json.load(open(os.path.join(GOLD, "qa_train_ref.json")))
    return {"cli": load_script("train_qa"), "gen": load_script("gen_qa_train_golden"), "meta": meta,
            "tok": transformers.BertTokenizer(os.path.join(ref.ASSETS, "vocab.txt"), do_lower_case=True)}


def run(env, feed_kind, dropout, extra=(), loss_scale="dynamic"):
    """scripts/train_qa.py's start-up (seeds, model, dataset, sampler, arena) and its train() with the golden run's flags; no evaluation, no
    files. Returns (train()'s result, the parameters as bytes, the index sequences the sampler drew)."""
    from multihop_dense_retrieval_amd import qa_train_arena, qa_train_data, reader_train
    cli, gen, tok = env["cli"], env["gen"], env["tok"]
    args = cli.train_args(gen.train_argv("electra-tiny", "", "", extra=("--eval-period", "-1") + tuple(extra)))
    assert args.sp_pred and args.output_dir == "" and args.seed == env["meta"]["seed"]
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

    if feed_kind == "arena":
        feed = cli.arena_batches(qa_train_arena.QATrainArena.from_dataset(ds).to("cuda"), tok.pad_token_id, torch.device("cuda", torch.cuda.current_device()))
    else:
        feed = cli.host_batches(ds, tok.pad_token_id, "cuda")
    out = cli.train(args, model, Recording(), feed, lambda: {"em": 0.0}, Quiet(), loss_scale=loss_scale)
    torch.cuda.synchronize()
    return out, {k: v.detach().cpu().numpy().tobytes() for k, v in model.state_dict().items()}, drawn


def test_arena_feed_and_host_feed_leave_the_same_bytes(env):
    a, pa, da = run(env, "arena", 0.1, ("--num_train_epochs", "2"))
    h, ph, dh = run(env, "host", 0.1, ("--num_train_epochs", "2"))
    assert da == dh and len(da) == 2 and a["global_step"] == h["global_step"] == 12
    assert a["loss"] == h["loss"] and len(a["loss"]) == 12
    assert list(pa) == list(ph)
    for k in pa:
        assert pa[k] == ph[k], (k, "the two feeds leave different parameters")
    start = ref.checkpoint(True)
    assert pa["encoder.encoder.layer.0.output.dense.weight"] != start["encoder.encoder.layer.0.output.dense.weight"].numpy().tobytes()


def test_first_loss_and_falling_epoch_means_against_the_reference_run(env):
    t = env["meta"]["train"]
    out, _, drawn = run(env, "arena", 0.0)
    assert drawn == t["drawn"]  # the reference script's own sampler, under its own seeding
    assert len(out["loss"]) == len(t["loss"]) == 18 and out["global_step"] == 18
    got, gold = out["loss"][0], t["loss"][0]
    rel = abs(got - gold) / abs(gold)
    print(f"first batch: loss {got:.6f}, reference {gold:.6f}, relative error {rel:.3e} (2^{np.log2(max(rel, 1e-30)):.2f})")
    print("epoch means", [round(x, 4) for x in out["epoch_means"]], "reference", [round(x, 4) for x in t["epoch_means"]], "steps skipped by the loss scale",
          out["skipped_steps"])
    assert rel <= FIRST_LOSS_REL
    assert t["epoch_means"][-1] < t["epoch_means"][0] and out["epoch_means"][-1] < out["epoch_means"][0]
    assert t["epochs"] == 3 and t["learning_rate"] == 1e-3  # the flags for which the reference's CPU run falls (recorded in the golden)
    # The dynamic loss scale starts at 2^16 and skips steps while it comes down, as apex's does; the reference's golden run is fp32 without one.
    # Under a fixed scale no step is skipped and the run is the reference's, step for step, up to fp16: the same sequences, all 18 steps taken.
    fixed, _, drawn = run(env, "arena", 0.0, loss_scale=256.0)
    print("fixed loss scale 256: epoch means", [round(x, 4) for x in fixed["epoch_means"]], "skipped", fixed["skipped_steps"])
    print("per batch", [round(x, 2) for x in fixed["loss"]], "reference", [round(x, 2) for x in t["loss"]])
    assert drawn == t["drawn"] and fixed["skipped_steps"] == 0 and out["skipped_steps"] > 0
    assert fixed["epoch_means"][-1] < fixed["epoch_means"][0]


def test_accumulation_takes_the_references_boundary_count(env):
    out, _, drawn = run(env, "arena", 0.0, ("--num_train_epochs", "2", "--gradient_accumulation_steps", "2"))
    n_batches = sum(-(-len(e) // 4) for e in drawn)
    boundaries = sum(1 for batch_step in range(1, n_batches + 1) if (batch_step + 1) % 2 == 0)  # train_qa.py:170, batch_step counted from 1
    assert n_batches == 12 and out["global_step"] == boundaries == 6
    # the meter is fed the DIVIDED loss, as the reference's is
    full, _, _ = run(env, "arena", 0.0, ("--num_train_epochs", "2"))
    assert abs(out["loss"][0] - full["loss"][0] / 2) <= 1e-6 * abs(full["loss"][0])
