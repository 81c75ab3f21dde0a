"""CPU: the reader's training item arena (multihop_dense_retrieval_amd/qa_train_arena.py): its numpy assembly equals the reference's
qa_collate on every golden batch (tests/golden/qa_train_ref.npz), batch_shape gives qa_collate's widths from host metadata, save / load
round-trips and a foreign tag is refused. include/mdr_reader_train.h, the binding table and the library agree. (The kernel:
tests/test_qa_train_assemble_gpu.py.)"""
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
def fixture_arena():
    import transformers
    from multihop_dense_retrieval_amd import qa_train_arena, qa_train_data
    meta = json.load(open(os.path.join(GOLD, "qa_train_ref.json")))
    tok = transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)
    ds = qa_train_data.QATrainDataset(tok, ITEMS, meta["max_seq_len"], meta["max_q_len"])
    return qa_train_arena.QATrainArena.from_dataset(ds), meta, np.load(os.path.join(GOLD, "qa_train_ref.npz")), tok, ds


def test_assemble_host_equals_every_reference_batch(fixture_arena):
    arena, meta, z, tok, _ = fixture_arena
    assert arena.n == len(meta["items"]) == 29
    first = meta["epochs"][0]
    for bi, lo in enumerate(range(0, len(first), meta["batch"])):
        idx = first[lo:lo + meta["batch"]]
        got = arena.assemble_host(idx, pad_id=tok.pad_token_id)
        keys = sorted(k.split(".", 1)[1] for k in z.files if k.startswith(f"b{bi}."))
        assert set(keys) <= set(got) and len(keys) == 10
        for k in keys:
            assert got[k].dtype == np.int64 and np.array_equal(got[k], z[f"b{bi}.{k}"]), (bi, k)
        assert arena.batch_shape(idx) == (z[f"b{bi}.input_ids"].shape[1], z[f"b{bi}.sent_offsets"].shape[1], z[f"b{bi}.starts"].shape[1])
        assert got["para_offsets"].tolist() == [meta["items"][i]["para_offset"] for i in idx]
        assert got["lengths"].tolist() == z[f"b{bi}.attention_mask"].sum(1).tolist()
    assert bi + 1 == meta["n_batches"]


def test_rows_outside_the_arena_are_empty_and_widths_cut(fixture_arena):
    arena = fixture_arena[0]
    got = arena.assemble_host([-1, 0, arena.n, 0], out_len=20, n_sent=2, n_span=2, pad_id=9)
    for r in (0, 2):
        assert (got["input_ids"][r] == 9).all() and not got["attention_mask"][r].any() and not got["token_type_ids"][r].any()
        assert not got["paragraph_mask"][r].any() and not got["sent_offsets"][r].any() and (got["starts"][r] == -1).all() and (got["ends"][r] == -1).all()
        assert got["label"][r, 0] == -1 and got["ans_covered"][r, 0] == 0 and got["lengths"][r] == 0 and got["para_offsets"][r] == 0
    full = arena.assemble_host([0])
    assert full["input_ids"].shape[1] == 39 and full["starts"].shape[1] == 3 and full["sent_offsets"].shape[1] == 3
    for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask"):
        assert np.array_equal(got[k][1], full[k][0, :20]) and np.array_equal(got[k][1], got[k][3])
    assert np.array_equal(got["starts"][1], full["starts"][0, :2]) and np.array_equal(got["sent_labels"][1], full["sent_labels"][0, :2])
    assert got["lengths"][1] == 39  # not clipped to out_len
    assert arena.batch_shape([-1, arena.n]) == (1, 0, 1) and arena.batch_shape([]) == (1, 0, 1)


def test_save_load_round_trips_and_a_foreign_tag_is_refused(fixture_arena, tmp_path):
    from multihop_dense_retrieval_amd import qa_train_arena
    arena, meta, _, tok, ds = fixture_arena
    train_file = str(tmp_path / "train.jsonl")
    with open(train_file, "wb") as f:
        f.write(open(ITEMS, "rb").read())
    tag = qa_train_arena.train_arena_tag(tok, meta["max_seq_len"], meta["max_q_len"], train_file)
    path = str(tmp_path / "a.npz")
    arena.save(path, tag=tag)
    back = qa_train_arena.QATrainArena.load(path, expect_tag=tag)
    for name, _ in qa_train_arena._ARRAYS:
        a, b = getattr(arena, name), getattr(back, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    for other in (qa_train_arena.train_arena_tag(tok, meta["max_seq_len"] + 1, meta["max_q_len"], train_file),
                  qa_train_arena.train_arena_tag(tok, meta["max_seq_len"], meta["max_q_len"] - 1, train_file), "qa-arena-v1|something else"):
        assert other != tag and qa_train_arena.QATrainArena.load(path, expect_tag=other) is None
    with open(train_file, "ab") as f:  # another size: another tag
        f.write(b"\n")
    assert qa_train_arena.train_arena_tag(tok, meta["max_seq_len"], meta["max_q_len"], train_file) != tag
    # load_or_build: builds and writes the cache, then reads it back; the cache of another cut is rebuilt, not reused
    with open(train_file, "wb") as f:
        f.write(open(ITEMS, "rb").read())
    calls = []
    one = qa_train_arena.QATrainArena.load_or_build(train_file, ds, tok, log=calls.append)
    two = qa_train_arena.QATrainArena.load_or_build(train_file, ds, tok, log=calls.append)
    assert len(calls) == 1 and os.path.exists(train_file + ".qa_train_arena.npz") and np.array_equal(one.tokens, two.tokens)


def test_bad_index_arrays_are_refused():
    from multihop_dense_retrieval_amd import qa_train_arena
    A = qa_train_arena.QATrainArena
    ok = dict(tokens=[5, 6, 7], offsets=[0, 2, 3], para_offset=[1, 1], sent_pos=[1], sent_label=[0], sent_index=[0, 1, 1], spans=[[-1, -1], [1, 1]],
              span_index=[0, 1, 2], label=[1, 0], ans_covered=[1, 0])
    assert A(**ok).bytes_per_item > 0
    for key, bad in (("offsets", [0, 2, 4]), ("offsets", [0, 3, 2]), ("sent_index", [0, 2, 1]), ("span_index", [0, 0, 2]), ("label", [1])):
        with pytest.raises(ValueError):
            A(**dict(ok, **{key: bad}))


def test_header_binding_and_library_agree():
    """include/mdr_reader_train.h declares exactly what qa_train_arena.SIGNATURES binds and the library exports, apart from every other
    header's table; the signature has the prototype's number of arguments; the native source reads no environment variable."""
    import importlib
    from multihop_dense_retrieval_amd import _lib, build, qa_train_arena
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdr_reader_train.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(qa_train_arena.SIGNATURES) == sorted(qa_train_arena.EXPORTED_SYMBOLS) == ["mdr_reader_train_assemble"]
    assert not set(declared) & set(_lib.EXPORTED_SYMBOLS)
    for mod, attr in (("attention", "SIGNATURES"), ("linear", "SIGNATURES"), ("layernorm", "SIGNATURES"), ("embedding", "SIGNATURES"), ("optim", "SIGNATURES"),
                      ("criterions", "SIGNATURES"), ("criterions", "LOSS_SIGNATURES"), ("reader", "SIGNATURES")):
        assert not set(declared) & set(getattr(importlib.import_module("multihop_dense_retrieval_amd." + mod), attr)), mod
    for name, (_, args) in qa_train_arena.SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args) == proto.count(",") + 1, name
    lib = ctypes.CDLL(build.build_lib())
    assert hasattr(lib, "mdr_reader_train_assemble")
    qa_train_arena.lib()
    src = open(os.path.join(ROOT, "multihop_dense_retrieval_amd", "csrc", "mdr_reader_train.hip")).read()
    assert "getenv" not in src
    for struct, cls in (("mdr_reader_train_arena", qa_train_arena.TrainArena), ("mdr_reader_train_batch", qa_train_arena.TrainBatch)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", text, flags=re.S).group(1)
        fields = re.findall(r"\b(\w+);", body)
        assert fields == [f[0] for f in cls._fields_], struct
