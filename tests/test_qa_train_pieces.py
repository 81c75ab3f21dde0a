"""CPU: the reader's training piece arena (multihop_dense_retrieval_amd/qa_train_pieces.py): its numpy composition equals the reference's
qa_collate on every golden batch (tests/golden/qa_train_ref.npz) and the item arena's assembly (qa_train_arena.QATrainArena.assemble_host)
item by item, with cut widths and on a list that repeats and permutes every item; batch_shape gives the same widths from host metadata;
the arrays do not depend on the worker count; chains of another length than two are refused; save / load round-trips and every change of
what the cache is valid for means a rebuild; three mutants of the composition are caught by the reference's own output.
include/mdr_reader_train_pieces.h, the binding table and the library agree. (The kernel: tests/test_qa_train_compose_gpu.py.)"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")
ITEMS = os.path.join(GOLD, "qa_train_items.jsonl")


@pytest.fixture(scope="module")
def fx():
    import transformers
    from multihop_dense_retrieval_amd import qa_train_arena, qa_train_data, qa_train_pieces
    meta = json.load(open(os.path.join(GOLD, "qa_train_ref.json")))
    tok = transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)
    ds = qa_train_data.QATrainDataset(tok, ITEMS, meta["max_seq_len"], meta["max_q_len"])
    return {"pieces": qa_train_pieces.QATrainPieces.from_dataset(ds), "items": qa_train_arena.QATrainArena.from_dataset(ds), "meta": meta,
            "z": np.load(os.path.join(GOLD, "qa_train_ref.npz")), "tok": tok, "ds": ds}


def first_epoch(meta):
    first = meta["epochs"][0]
    return [(bi, first[lo:lo + meta["batch"]]) for bi, lo in enumerate(range(0, len(first), meta["batch"]))]


def golden_keys(z, bi):
    return sorted(k.split(".", 1)[1] for k in z.files if k.startswith(f"b{bi}."))


def assert_same(got, want, where):
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        assert got[k].dtype == w.dtype == np.int64 and got[k].shape == w.shape and np.array_equal(got[k], w), (where, k)


def test_compose_host_equals_every_reference_batch(fx):
    pieces, meta, z, tok = fx["pieces"], fx["meta"], fx["z"], fx["tok"]
    batches = first_epoch(meta)
    assert len(batches) == meta["n_batches"]
    for bi, idx in batches:
        got = pieces.compose_host(idx, pad_id=tok.pad_token_id)
        keys = golden_keys(z, bi)
        assert set(keys) <= set(got) and len(keys) == 10
        for k in keys:
            assert got[k].dtype == np.int64 and np.array_equal(got[k], z[f"b{bi}.{k}"]), (bi, k)
        assert pieces.batch_shape(idx) == (z[f"b{bi}.input_ids"].shape[1], z[f"b{bi}.sent_offsets"].shape[1], z[f"b{bi}.starts"].shape[1])
        assert got["para_offsets"].tolist() == [meta["items"][i]["para_offset"] for i in idx]
        assert got["lengths"].tolist() == z[f"b{bi}.attention_mask"].sum(1).tolist()


def test_compose_host_equals_the_item_arena(fx):
    pieces, items = fx["pieces"], fx["items"]
    n = items.n
    for i in range(n):
        assert_same(pieces.compose_host([i]), items.assemble_host([i]), i)
    outside = [-1, 0, n, 0]
    assert_same(pieces.compose_host(outside, out_len=20, n_sent=2, n_span=2, pad_id=9), items.assemble_host(outside, out_len=20, n_sent=2, n_span=2, pad_id=9), "cut")
    rng = np.random.default_rng(3)
    mixed = list(rng.permutation(n)) + list(rng.permutation(n)[:7]) + list(range(n))  # every item, repeated and permuted
    assert sorted(set(mixed)) == list(range(n))
    assert_same(pieces.compose_host(mixed, pad_id=3), items.assemble_host(mixed, pad_id=3), "mixed")
    for idx in ([i] for i in range(n)):
        assert pieces.batch_shape(idx) == items.batch_shape(idx)
    for idx in (outside, mixed, [], [-1, n]):
        assert pieces.batch_shape(idx) == items.batch_shape(idx), idx
    assert pieces.batch_shape([]) == (1, 0, 1)


def test_counts_are_the_distinct_questions_and_passages(fx):
    from multihop_dense_retrieval_amd import qa_arena
    pieces, ds = fx["pieces"], fx["ds"]
    texts = [qa_arena.passage_text(p) for rec in ds.data for p in rec["passages"]]
    assert pieces.n == 29 and pieces.n_questions == len({rec["qid"] for rec in ds.data}) == 9
    assert len(texts) == 58 and pieces.n_passages == len(set(texts)) == 48
    assert pieces.bytes_per_item > 0 and pieces.items.shape == (29, 5) and int(pieces.items[:, 4].sum()) == 11
    assert pieces.max_seq_len == 48 and pieces.max_q_len == 24


def test_arrays_do_not_depend_on_the_worker_count(fx):
    from multihop_dense_retrieval_amd import qa_train_pieces
    two = qa_train_pieces.QATrainPieces.from_dataset(fx["ds"], workers=2)
    for name, _ in qa_train_pieces._ARRAYS:
        a, b = getattr(fx["pieces"], name), getattr(two, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize("length", [1, 3])
def test_a_chain_of_another_length_is_refused(fx, length):
    import copy
    import types
    from multihop_dense_retrieval_amd import qa_train_pieces
    ds = fx["ds"]
    data = copy.deepcopy(ds.data[:5])
    data[3]["passages"] = (data[3]["passages"] + data[0]["passages"])[:length]
    other = types.SimpleNamespace(data=data, tokenizer=ds.tokenizer, max_seq_len=ds.max_seq_len, max_q_len=ds.max_q_len, simple_tok=ds.simple_tok)
    with pytest.raises(ValueError, match=rf"record 3 .*chain of {length} passages"):
        qa_train_pieces.QATrainPieces.from_dataset(other)


def test_cache_round_trips_and_is_rebuilt_for_anything_else(fx, tmp_path):
    from multihop_dense_retrieval_amd import qa_train_arena, qa_train_data, qa_train_pieces
    pieces, meta, tok, ds = fx["pieces"], fx["meta"], fx["tok"], fx["ds"]
    P = qa_train_pieces.QATrainPieces
    train_file = str(tmp_path / "train.jsonl")

    def write(extra=b""):
        with open(train_file, "wb") as f:
            f.write(open(ITEMS, "rb").read() + extra)

    write()
    tag = qa_train_pieces.train_pieces_tag(tok, meta["max_seq_len"], meta["max_q_len"], train_file)
    assert tag != qa_train_arena.train_arena_tag(tok, meta["max_seq_len"], meta["max_q_len"], train_file)  # a rule string of its own
    assert tag.split("|", 1)[1] == qa_train_arena.train_arena_tag(tok, meta["max_seq_len"], meta["max_q_len"], train_file).split("|", 1)[1]
    path = str(tmp_path / "a.npz")
    pieces.save(path, tag=tag)
    back = P.load(path, expect_tag=tag)
    for name, _ in qa_train_pieces._ARRAYS:
        a, b = getattr(pieces, name), getattr(back, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert_same(back.compose_host(list(range(back.n))), pieces.compose_host(list(range(pieces.n))), "loaded")
    for other in (qa_train_pieces.train_pieces_tag(tok, meta["max_seq_len"] + 1, meta["max_q_len"], train_file),
                  qa_train_pieces.train_pieces_tag(tok, meta["max_seq_len"], meta["max_q_len"] - 1, train_file),
                  qa_train_arena.train_arena_tag(tok, meta["max_seq_len"], meta["max_q_len"], train_file), "qa-arena-v1|something else"):
        assert other != tag and P.load(path, expect_tag=other) is None
    # load_or_build: builds once and writes the cache, loads the second time
    calls = []
    one = P.load_or_build(train_file, ds, tok, log=calls.append)
    assert len(calls) == 1 and calls[0].startswith("Preparing") and os.path.exists(train_file + ".qa_train_pieces.npz")
    two = P.load_or_build(train_file, ds, tok, log=calls.append, workers=2)
    assert len(calls) == 2 and calls[1].startswith("Loaded") and np.array_equal(one.p_tokens, two.p_tokens) and np.array_equal(one.items, two.items)
    assert not [n for n in os.listdir(str(tmp_path)) if ".tmp" in n]  # written under a temporary name and renamed
    builds = lambda: sum(c.startswith("Preparing") for c in calls)  # noqa: E731
    # another max_seq_len, another max_q_len: a rebuild each
    for seq, q in ((meta["max_seq_len"] + 1, meta["max_q_len"]), (meta["max_seq_len"], meta["max_q_len"] - 1)):
        before = builds()
        other_ds = qa_train_data.QATrainDataset(tok, train_file, seq, q)
        got = P.load_or_build(train_file, other_ds, tok, log=calls.append)
        assert builds() == before + 1 and (got.max_seq_len, got.max_q_len) == (seq, q)
    before = builds()
    P.load_or_build(train_file, ds, tok, log=calls.append)  # (the cache now holds the other cut)
    assert builds() == before + 1
    # a grown train file: another tag, and another item count
    write(open(ITEMS, "rb").read().split(b"\n")[0] + b"\n")
    grown = qa_train_data.QATrainDataset(tok, train_file, meta["max_seq_len"], meta["max_q_len"])
    assert qa_train_pieces.train_pieces_tag(tok, meta["max_seq_len"], meta["max_q_len"], train_file) != tag and len(grown) > len(ds)
    before = builds()
    assert P.load_or_build(train_file, grown, tok, log=calls.append).n == len(grown) and builds() == before + 1
    # a foreign tag in the cache file
    pieces.save(train_file + ".qa_train_pieces.npz", tag="someone else's")
    before = builds()
    assert P.load_or_build(train_file, grown, tok, log=calls.append).n == len(grown) and builds() == before + 1
    # the right tag over another item count
    pieces.save(train_file + ".qa_train_pieces.npz", tag=qa_train_pieces.train_pieces_tag(tok, meta["max_seq_len"], meta["max_q_len"], train_file))
    before = builds()
    assert P.load_or_build(train_file, grown, tok, log=calls.append).n == len(grown) and builds() == before + 1


def misses(fx, **mutant):
    """The first-epoch golden batches that compose_host under `mutant` does not reproduce."""
    out = []
    for bi, idx in first_epoch(fx["meta"]):
        got = fx["pieces"].compose_host(idx, pad_id=fx["tok"].pad_token_id, **mutant)
        if any(got[k].shape != fx["z"][f"b{bi}.{k}"].shape or not np.array_equal(got[k], fx["z"][f"b{bi}.{k}"]) for k in golden_keys(fx["z"], bi)):
            out.append(bi)
    return out


def test_span_mutants_miss_a_golden_batch(fx):
    assert misses(fx) == []
    assert misses(fx, drop_cut=False), "spans behind the cut kept: no golden batch noticed"
    assert misses(fx, clamp_end=False), "span ends not clamped: no golden batch noticed"


def test_sentence_label_mutant_misses_the_references_rows(fx):
    """Labels indexed per passage and not by the chain's sentence ordinal. The reference's own rows catch it (tests/golden/qa_train_ref.npz,
    item<i>.sent_labels: QADataset(train=True).__getitem__ of every item), on the gold chains whose second passage is labelled differently
    from the start of the first inside the cut: t5's (item 13: labels 1 | 0 1). The first epoch's BATCHES do not: the sampler's multiple-of-8
    cut leaves t5 out of that epoch, and the other gold chains that would tell (t2, t3) lose their second passage's sentences to the cut at
    48 -- measured: misses(labels_per_passage=True) == [] -- so this mutant is held against the per-item rows, and the batches are asserted
    to be blind to it so that a fixture that starts to see it is noticed."""
    pieces, z, meta = fx["pieces"], fx["z"], fx["meta"]
    caught = []
    for i in range(pieces.n):
        want = z[f"item{i}.sent_labels"]
        right = pieces.compose_host([i])["sent_labels"][0]
        assert np.array_equal(right, want), i  # the composition itself reproduces every item's row
        wrong = pieces.compose_host([i], labels_per_passage=True)["sent_labels"][0]
        if not np.array_equal(wrong, want):
            caught.append(i)
    assert 13 in caught and all(meta["items"][i]["label"] == 1 for i in caught), caught
    assert misses(fx, labels_per_passage=True) == [] and 13 not in meta["epochs"][0]


def test_bad_arrays_are_refused():
    from multihop_dense_retrieval_amd import qa_train_pieces
    P = qa_train_pieces.QATrainPieces
    ok = dict(q_tokens=[5, 6, 7], q_offsets=[0, 2, 3], p_tokens=[1, 2, 3, 4, 5], p_offsets=[0, 3, 5], p_sent_starts=[0, 2, 1], p_sent_offsets=[0, 2, 3],
              items=[[0, 0, 1, 1, 1], [1, 1, 1, 0, 0]], sent_label=[1, 0, 1], sent_label_index=[0, 3, 3], spans=[[0, 0], [5, 9]], span_index=[0, 2, 2],
              special=[101, 102, 7, 8], cuts=[16, 4])
    a = P(**ok)
    assert a.bytes_per_item > 0 and (a.n, a.n_questions, a.n_passages) == (2, 2, 2)
    assert a.lens.tolist() == [4 + 9 + 1, 3 + 8 + 1] and a.n_sents.tolist() == [3, 2] and a.n_spans.tolist() == [2, 1]
    for key, bad in (("q_offsets", [0, 2, 4]), ("q_offsets", [0, 3, 2]), ("p_offsets", [0, 3, 6]), ("p_sent_offsets", [0, 4, 3]), ("span_index", [0, 1, 3]),
                     ("sent_label_index", [0, 2, 3]),  # neither none nor one label per sentence of the chain
                     ("items", [[0, 0, 2, 1, 1], [1, 1, 1, 0, 0]]), ("items", [[2, 0, 1, 1, 1], [1, 1, 1, 0, 0]]), ("items", [[0, -1, 1, 1, 1], [1, 1, 1, 0, 0]]),
                     ("p_sent_starts", [2, 0, 1]), ("p_sent_starts", [0, 3, 1]), ("cuts", [7, 4]), ("special", [1, 2, 3])):
        with pytest.raises(ValueError):
            P(**dict(ok, **{key: bad}))


def test_header_binding_and_library_agree():
    """include/mdr_reader_train_pieces.h declares exactly what qa_train_pieces.SIGNATURES binds and the library exports, apart from every
    other header's table; the signature has the prototype's number of arguments; the struct's fields are the binding's; the batch struct is
    include/mdr_reader_train.h's, included and not copied; the native source reads no environment variable."""
    import importlib
    from multihop_dense_retrieval_amd import _lib, build, qa_train_arena, qa_train_pieces
    raw = open(os.path.join(ROOT, "include", "mdr_reader_train_pieces.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(qa_train_pieces.SIGNATURES) == sorted(qa_train_pieces.EXPORTED_SYMBOLS) == ["mdr_reader_train_compose"]
    assert not set(declared) & set(_lib.EXPORTED_SYMBOLS) and not set(declared) & set(qa_train_arena.SIGNATURES)
    for mod, attr in (("attention", "SIGNATURES"), ("linear", "SIGNATURES"), ("layernorm", "SIGNATURES"), ("embedding", "SIGNATURES"), ("optim", "SIGNATURES"),
                      ("criterions", "SIGNATURES"), ("criterions", "LOSS_SIGNATURES"), ("reader", "SIGNATURES")):
        assert not set(declared) & set(getattr(importlib.import_module("multihop_dense_retrieval_amd." + mod), attr)), mod
    for name, (_, args) in qa_train_pieces.SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args) == proto.count(",") + 1, name
        assert [a.strip() for a in proto.split(",")][-2:] == ["int device", "void* stream"]
    lib = ctypes.CDLL(build.build_lib())
    assert hasattr(lib, "mdr_reader_train_compose")
    qa_train_pieces.lib()
    src = open(os.path.join(ROOT, "multihop_dense_retrieval_amd", "csrc", "mdr_reader_train_pieces.hip")).read()
    assert "getenv" not in src
    body = re.search(r"typedef struct mdr_reader_train_pieces \{(.*?)\} mdr_reader_train_pieces;", text, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", body) == [f[0] for f in qa_train_pieces.TrainPieces._fields_]
    assert '#include "mdr_reader_train.h"' in text and "typedef struct mdr_reader_train_batch" not in text
    assert qa_train_pieces.TrainBatch is qa_train_arena.TrainBatch
