"""CPU: the reader's training data path (multihop_dense_retrieval_amd/qa_train_data.py) against the reference's own QADataset(train=True),
MhopSampler and qa_collate, executed by scripts/gen_qa_train_golden.py on tests/golden/qa_train_items.jsonl (tests/golden/qa_train_ref.*).
Every quirk DESIGN.md §27 lists is pinned twice: the mirror equals the golden, and a mutant without the quirk misses it."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")
ITEMS = os.path.join(GOLD, "qa_train_items.jsonl")
FIELDS = ("input_ids", "token_type_ids", "attention_mask", "paragraph_mask", "starts", "ends", "sent_offsets", "sent_labels", "ans_covered", "label")


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLD, "qa_train_ref.json"))), np.load(os.path.join(GOLD, "qa_train_ref.npz"))


@pytest.fixture(scope="module")
def tok():
    import transformers
    return transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)


def dataset(tok, meta, cls=None):
    from multihop_dense_retrieval_amd import qa_train_data as td
    return (cls or td.QATrainDataset)(tok, ITEMS, meta["max_seq_len"], meta["max_q_len"])


def fields_of(it):
    out = {k: it["encodings"][k].view(-1) for k in FIELDS[:3]}
    out.update({k: it[k].view(-1) for k in FIELDS[3:]})
    return {k: v.numpy().astype(np.int64) for k, v in out.items()}


def items_differ(ds, z):
    """indices of the items that differ from the golden in any field"""
    bad = []
    for i in range(len(ds)):
        f = fields_of(ds[i])
        if any(f[k].shape != z[f"item{i}.{k}"].shape or not np.array_equal(f[k], z[f"item{i}.{k}"]) for k in FIELDS):
            bad.append(i)
    return bad


def test_every_item_equals_the_reference_field_for_field(gold, tok):
    meta, z = gold
    ds = dataset(tok, meta)
    assert len(ds) == len(meta["items"])
    assert {k: list(v) for k, v in ds.qid2gold.items()} == meta["qid2gold"] and {k: list(v) for k, v in ds.qid2neg.items()} == meta["qid2neg"]
    for i, rec in enumerate(meta["items"]):
        it = ds[i]
        assert (it["qid"], it["para_offset"], len(it["wp_tokens"])) == (rec["qid"], rec["para_offset"], rec["n_wp"]), i
        f = fields_of(it)
        for k in FIELDS:
            assert f[k].shape == z[f"item{i}.{k}"].shape and np.array_equal(f[k], z[f"item{i}.{k}"]), (i, k, f[k], z[f"item{i}.{k}"])
    assert items_differ(ds, z) == []
    # reading an item twice gives the same fields (the records are not written to)
    assert all(np.array_equal(fields_of(ds[4])[k], z[f"item4.{k}"]) for k in FIELDS)


def test_the_toy_file_shows_every_case(gold):
    """the fixture's cases, read from the REFERENCE's output: three occurrences, a clamped end, a span behind the cut, a distant-supervised
    negative, a comparison negative that shares a gold title, yes / no, fewer and more negatives than neg_num, markers behind the cut, a
    non-ASCII answer."""
    meta, z = gold
    rec = meta["items"]
    st = [z[f"item{i}.starts"].tolist() for i in range(len(rec))]
    en = [z[f"item{i}.ends"].tolist() for i in range(len(rec))]
    cov = [int(z[f"item{i}.ans_covered"][0]) for i in range(len(rec))]
    nso = [len(z[f"item{i}.sent_offsets"]) for i in range(len(rec))]
    by = lambda qid, label: [i for i, r in enumerate(rec) if r["qid"] == qid and r["label"] == label]  # noqa: E731
    assert len(meta["qid2gold"]) == 9
    assert len(st[by("t1", 1)[0]]) == 3
    g2 = by("t2", 1)[0]
    assert rec[g2]["n_wp"] < rec[g2]["n_wp_uncut"] and st[g2] == en[g2] == [rec[g2]["para_offset"] + rec[g2]["n_wp"] - 1]  # "rock band": the end clamped
    assert st[by("t3", 1)[0]] == [-1] and nso[by("t3", 1)[0]] < rec[by("t3", 1)[0]]["n_sent_uncut"]
    assert [cov[i] for i in by("t1", 0)] == [1, 0, 0] and st[by("t1", 0)[0]] != [-1]
    assert [cov[i] for i in by("t4", 0)] == [0, 0] and [cov[i] for i in by("t9", 0)] == [0, 1]
    assert st[by("t5", 1)[0]] == [rec[by("t5", 1)[0]]["para_offset"]] and st[by("t6", 1)[0]] == [rec[by("t6", 1)[0]]["para_offset"] + 1]
    assert len(by("t7", 0)) == 1 < meta["neg_num"] < len(by("t8", 0)) == 4
    assert en[by("t8", 1)[0]][0] == st[by("t8", 1)[0]][0] + 1  # "Café Zürich": two WordPieces, matched through NFD
    assert all((z[f"item{i}.sent_labels"] == 0).all() for i, r in enumerate(rec) if r["label"] == 0)


def epochs_of(ds, meta, **kw):
    from multihop_dense_retrieval_amd import qa_train_data as td
    random.seed(meta["seed"])
    sampler = kw.pop("cls", td.MhopSampler)(ds, num_neg=meta["neg_num"], **kw)
    return sampler, [list(iter(sampler)) for _ in range(3)]


def test_sampler_len_and_three_epochs_equal_the_reference(gold, tok):
    from multihop_dense_retrieval_amd import qa_train_data as td
    meta, _ = gold
    sampler, epochs = epochs_of(dataset(tok, meta), meta)
    assert len(sampler) == meta["sampler_len"] == 24
    assert epochs == meta["epochs"]
    assert all(len(e) in (22, 23) for e in epochs)  # 8 of 9 questions, one of which has a single negative: fewer rows than len says
    assert td.loader_len(sampler, meta["batch"]) == meta["loader_len"] == 6
    # t_total: the reference's, from len(loader) -- more than the optimizer steps three epochs really take (batch size 1 shows every row)
    assert td.total_steps(sampler, 1, 1, 3.0) == 72.0 > 3 * len(td.epoch_batches(sampler, 1))


def test_collate_equals_the_reference_batches(gold, tok):
    from multihop_dense_retrieval_amd import qa_train_data as td
    meta, z = gold
    ds = dataset(tok, meta)
    first = meta["epochs"][0]
    batches = [first[lo:lo + meta["batch"]] for lo in range(0, len(first), meta["batch"])]
    assert len(batches) == meta["n_batches"] and len(batches[-1]) < meta["batch"]  # the last batch is short
    for bi, idx in enumerate(batches):
        net = td.qa_train_collate([ds[i] for i in idx], pad_id=tok.pad_token_id)["net_inputs"]
        keys = sorted(k.split(".", 1)[1] for k in z.files if k.startswith(f"b{bi}."))
        assert sorted(net) == keys
        for k in keys:
            assert np.array_equal(net[k].numpy().astype(np.int64), z[f"b{bi}.{k}"]), (bi, k)


# ---- mutants: each drops one quirk and must miss the golden --------------------------------------------------------------------------------


def test_mutant_negatives_shuffled_on_a_copy(gold, tok):
    from multihop_dense_retrieval_amd import qa_train_data as td
    meta, _ = gold

    class Copying(td.MhopSampler):
        def negatives_of(self, qid):
            neg = list(self.qid2neg[qid])
            random.shuffle(neg)
            return neg

    _, epochs = epochs_of(dataset(tok, meta), meta, cls=Copying)
    assert epochs[0] == meta["epochs"][0] and epochs[1:] != meta["epochs"][1:]  # the first epoch cannot tell; the later ones do


def test_mutant_n_gpu_one(gold, tok):
    meta, _ = gold
    sampler, epochs = epochs_of(dataset(tok, meta), meta, n_gpu=1)
    assert len(sampler) == 27 != meta["sampler_len"] and epochs != meta["epochs"]


def test_mutant_span_end_unclamped_and_cut_spans_kept(gold, tok):
    from multihop_dense_retrieval_amd import qa_train_data as td
    meta, z = gold

    class Unclamped(td.QATrainDataset):
        cut_spans = staticmethod(lambda spans, n_wp, po: td.cut_spans(spans, n_wp, po, clamp_end=False))

    class Kept(td.QATrainDataset):
        cut_spans = staticmethod(lambda spans, n_wp, po: td.cut_spans(spans, n_wp, po, drop_cut=False))

    rec = meta["items"]
    gold_of = lambda qid: [i for i, r in enumerate(rec) if r["qid"] == qid and r["label"] == 1][0]  # noqa: E731
    assert items_differ(dataset(tok, meta, Unclamped), z) == [gold_of("t2")]
    assert items_differ(dataset(tok, meta, Kept), z) == [gold_of("t3")]


def test_mutant_ans_covered_ignored_for_negatives(gold, tok):
    from multihop_dense_retrieval_amd import qa_train_data as td
    meta, z = gold

    class Never(td.QATrainDataset):
        negative_ans_covered = staticmethod(lambda bridge, titles, ans_titles: 0)

    class Always(td.QATrainDataset):
        negative_ans_covered = staticmethod(lambda bridge, titles, ans_titles: int(len(titles & ans_titles) > 0 or not bridge))

    cov1 = [i for i, r in enumerate(meta["items"]) if r["label"] == 0 and int(z[f"item{i}.ans_covered"][0]) == 1]
    assert len(cov1) == 2 and items_differ(dataset(tok, meta, Never), z) == cov1
    assert items_differ(dataset(tok, meta, Always), z) != []  # a comparison question's negative is never covered


def test_mutant_t_total_from_the_real_step_count(gold, tok):
    """The schedule the reference builds ends ABOVE zero: t_total counts neg_num + 1 rows per question."""
    from multihop_dense_retrieval_amd import optim, qa_train_data as td
    meta, _ = gold
    sampler, epochs = epochs_of(dataset(tok, meta), meta)
    bs, n_epochs = 1, 3.0  # (at batch size 1 every missing row is a missing step; at 4 the rounding up to whole batches hides one row)
    t_total = td.total_steps(sampler, bs, 1, n_epochs)
    real = sum(-(-len(e) // bs) for e in epochs)
    assert t_total == 72.0 and real < t_total
    assert optim.linear_schedule_with_warmup(real, t_total * 0.1, t_total) > 0.0  # the last step's factor under the reference's t_total
    assert optim.linear_schedule_with_warmup(real, real * 0.1, float(real)) == 0.0  # the mutant's reaches zero


def test_answer_matching_helpers():
    from multihop_dense_retrieval_amd import qa_train_data as td
    st = td.SimpleTokenizer()
    assert [t[0] for t in st.tokenize("Mr. O'Neil, 12-3!")] == ["Mr", ".", "O", "'", "Neil", ",", "12", "-", "3", "!"]
    assert td.para_has_answer(["new york"], "He lives in New  York.", st) and not td.para_has_answer(["york new"], "New York", st)
    assert td.match_answer_span("a New  York b new york", ["New York"], st) == ["New  York", "new york"]
    assert td.para_has_answer(["Café"], "the café is", st)  # both sides NFD-normalised
    assert td.match_answer_span("the café is", ["Café"], st) == []  # the context is not normalised here: precomposed text misses (kept)


# ---- the CLI's refusals ---------------------------------------------------------------------------------------------------------------------


def run_cli(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_qa.py"), *argv], capture_output=True, text=True, timeout=300)


def test_cli_names_the_missing_device_for_an_electra_directory(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    model_dir = tmp_path / "electra-tiny"
    model_dir.mkdir()
    for n in ("config.json", "vocab.txt"):
        (model_dir / n).write_bytes(open(os.path.join(ASSETS, n), "rb").read())
    r = run_cli("--do_train", "--model_name", str(model_dir), "--train_file", ITEMS, "--predict_file", ITEMS, "--output_dir", str(tmp_path / "logs"))
    assert r.returncode != 0 and "training is not supported: " in r.stderr and "HIP device" in r.stderr, r.stderr
    assert not (tmp_path / "logs").exists()  # refused before anything was opened


def test_cli_refuses_a_missing_train_file_and_the_default_model(tmp_path):
    r = run_cli("--do_train", "--output_dir", str(tmp_path / "logs"))
    assert r.returncode != 0 and r.stderr.strip().startswith("training is not supported: ") and "bert-base-uncased" in r.stderr
    assert not (tmp_path / "logs").exists()
