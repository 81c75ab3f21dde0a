"""CPU: the retriever's training token arena (multihop_dense_retrieval_amd/mhop_arena.py) against the reference's own runs on toy assets,
tests/golden/mhop_train_ref.{json,npz} (the interleaved eval and train reads of a --do_train run and every collated train batch) and
tests/golden/mhop_eval_ref.{json,npz} (every collated dev batch of a --do_predict run): choose() + assemble_host() give the reference's
batches and leave the generator where the dataset classes leave it; four wrong orders of the draws miss the golden; the rows' structure;
the cache and the refusals; include/mdr_mhop_train.h, the binding table and the library agree. (The kernel: tests/test_mhop_assemble_gpu.py.)"""
import ctypes
import importlib.util
import json
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def load_script(name):
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    spec = importlib.util.spec_from_file_location(name, os.path.join(scripts, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """The assets of tests/test_train_host.py::test_replayed_items_reproduce_every_collated_train_batch, and both fixtures."""
    from multihop_dense_retrieval_amd import data
    tmp = str(tmp_path_factory.mktemp("mhop_arena"))
    gen, tgen = load_script("gen_mhop_eval_golden"), load_script("gen_mhop_train_golden")
    a = gen.build_assets(tmp)
    meta = json.load(open(os.path.join(GOLD, "mhop_train_ref.json")))
    emeta = json.load(open(os.path.join(GOLD, "mhop_eval_ref.json")))
    assert meta["samples"] == tgen.train_samples() and emeta["samples"] == a["samples"]
    train_file = os.path.join(tmp, "train.jsonl")
    tgen.write_train_file(train_file, meta["samples"])
    lens = (meta["max_q_len"], meta["max_q_sp_len"], meta["max_c_len"])
    assert lens == (emeta["max_q_len"], emeta["max_q_sp_len"], emeta["max_c_len"]) and meta["seed"] == emeta["seed"]
    return {"tok": data.load_tokenizer(a["model_dir"]), "files": {"eval": a["dev"], "train": train_file}, "lens": lens, "meta": meta, "emeta": emeta,
            "npz": np.load(os.path.join(GOLD, "mhop_train_ref.npz")), "enpz": np.load(os.path.join(GOLD, "mhop_eval_ref.npz")), "tmp": tmp}


def datasets(env):
    from multihop_dense_retrieval_amd import mhop_data
    return {"eval": mhop_data.MhopDataset(env["tok"], env["files"]["eval"], *env["lens"]),
            "train": mhop_data.MhopTrainDataset(env["tok"], env["files"]["train"], *env["lens"])}


def arenas(env, cls=None):
    from multihop_dense_retrieval_amd import mhop_arena
    cls = cls or {}
    return {tag: cls.get(tag, mhop_arena.MhopArena).from_dataset(ds) for tag, ds in datasets(env).items()}


def replay(ar, items, batch):
    """The fixture's (dataset, index) reads through the arenas' choose(), grouped as the run grouped them: a pass over a set, in batches of
    batch[tag]. Returns {tag: [(assemble_host's batch, choose's widths), ...]}."""
    out, pending = {"eval": [], "train": []}, []
    for k, (tag, index) in enumerate(items):
        pending.append(index)
        if len(pending) == ar[tag].n or k + 1 == len(items) or items[k + 1][0] != tag:
            for lo in range(0, len(pending), batch[tag]):
                table, widths = ar[tag].choose(pending[lo:lo + batch[tag]])
                out[tag].append((ar[tag].assemble_host(table, widths), widths))
            pending = []
    return out


def misses(env, ar_train_run, ar_eval_run):
    """What of the two goldens a pair of arenas (one pair per reference run: each run starts from unread data) does NOT reproduce."""
    from multihop_dense_retrieval_amd import mhop_arena
    meta, emeta, missed = env["meta"], env["emeta"], []
    random.seed(meta["seed"])
    got = replay(ar_train_run, meta["items"], {"train": meta["train_batch"], "eval": emeta["batch"]})["train"]
    if len(got) != meta["n_train_batches"]:
        missed.append(("train", "batches", len(got)))
    for bi, (b, widths) in enumerate(got):
        for k, key in enumerate(mhop_arena.KEYS):
            want = env["npz"][f"t{bi}.{key}"]
            if b[key].shape != want.shape or not np.array_equal(b[key], want) or widths[k // 2] != want.shape[1]:
                missed.append(("train", bi, key))
    random.seed(emeta["seed"])
    got = replay(ar_eval_run, [["eval", i] for i in range(emeta["n_samples"])], {"eval": emeta["batch"]})["eval"]
    for bi, (b, widths) in enumerate(got):
        for k, key in enumerate(mhop_arena.KEYS):
            want = env["enpz"][f"b{bi}.{key}"]
            if b[key].shape != want.shape or not np.array_equal(b[key], want) or widths[k // 2] != want.shape[1]:
                missed.append(("eval", bi, key))
    return missed


def test_assemble_host_equals_every_reference_batch(env):
    from multihop_dense_retrieval_amd import mhop_arena
    meta, emeta = env["meta"], env["emeta"]
    keys = sorted(k.split(".", 1)[1] for k in env["npz"].files if k.startswith("t0."))
    assert keys == sorted(mhop_arena.KEYS) == sorted(k.split(".", 1)[1] for k in env["enpz"].files if k.startswith("b0.") and ".emb." not in k)
    assert {tag for tag, _ in meta["items"]} == {"eval", "train"} and meta["items"][0][0] != meta["items"][-1][0]  # the reads interleave
    state = random.getstate()
    ar = arenas(env)
    assert random.getstate() == state  # building draws nothing
    assert ar["train"].train and not ar["eval"].train and ar["train"].n == 23 and ar["eval"].n == emeta["n_samples"] == 24
    assert misses(env, ar, {"eval": arenas(env)["eval"]}) == []
    # every dtype is mhop_collate's, and the generator ends where the dataset classes leave it after the same reads from the same seed
    random.seed(meta["seed"])
    ar = arenas(env)
    got = replay(ar, meta["items"], {"train": meta["train_batch"], "eval": emeta["batch"]})
    assert len(got["train"]) == meta["n_train_batches"] and len(got["eval"]) == meta["epochs"] * emeta["n_batches"]
    assert all(v.dtype == np.int64 for b, _ in got["train"] + got["eval"] for v in b.values())
    after_arena = random.getstate()
    random.seed(meta["seed"])
    sets = datasets(env)
    for tag, index in meta["items"]:
        sets[tag][index]
    assert random.getstate() == after_arena
    # and the orders the arena kept are the orders the datasets' lists are in
    unread = datasets(env)
    for tag in ("eval", "train"):
        for i, (now, was) in enumerate(zip(sets[tag].data, unread[tag].data)):
            assert [p["title"] for p in now["pos_paras"]] == [was["pos_paras"][k]["title"] for k in ar[tag].pos_order[i]]
            assert [p["title"] for p in now["neg_paras"]] == [was["neg_paras"][k]["title"] for k in ar[tag].neg_order[i]]


def mutants():
    from multihop_dense_retrieval_amd.mhop_arena import MhopArena

    class NegativesOnACopy(MhopArena):  # the negative order is shuffled on a copy, not cumulatively
        def draw(self, i):
            out = super().draw(i)
            self.neg_order[i].sort()
            return out

    class NoShuffleAtEval(MhopArena):  # the comparison shuffle is skipped at eval time
        def draw(self, i):
            if self.train or self.start[i] >= 0:
                return super().draw(i)
            return 0, self.neg_order[i][0], self.neg_order[i][1]

    class NegativesFirst(MhopArena):  # the negatives are shuffled before the positives
        def draw(self, i):
            negs = self.neg_order[i]
            if self.train:
                random.shuffle(negs)
            if self.start[i] < 0:
                random.shuffle(self.pos_order[i])
                return self.pos_order[i][0], negs[0], negs[1]
            return int(self.start[i]), negs[0], negs[1]

    class FirstPositiveQsp(MhopArena):  # q_sp always uses the first positive
        def choose(self, indices):
            table, _ = super().choose(indices)
            table[:, 1] = [self.qsp_rows[int(i), 0] for i in indices]
            return table, self.widths(table)

    return {"negatives_on_a_copy": ({"train": NegativesOnACopy}, "train"), "no_shuffle_at_eval": ({"eval": NoShuffleAtEval}, "eval"),
            "negatives_first": ({"train": NegativesFirst}, "train"), "first_positive_q_sp": ({"train": FirstPositiveQsp, "eval": FirstPositiveQsp}, "both")}


@pytest.mark.parametrize("name", ["negatives_on_a_copy", "no_shuffle_at_eval", "negatives_first", "first_positive_q_sp"])
def test_wrong_draws_miss_the_golden(env, name):
    base = arenas(env)
    assert (base["train"].start < 0).any() and (base["eval"].start < 0).any()  # each set holds a comparison sample: both shuffles are exercised
    assert (base["train"].start >= 0).any() and int(np.diff(base["train"].neg_index).max()) > 2  # and a shuffle of the negatives can show
    cls, where = mutants()[name]
    missed = misses(env, arenas(env, cls), {"eval": arenas(env, cls)["eval"]})
    assert missed, f"the golden does not tell {name} from the reference's order"
    if where == "train":
        assert any(m[0] == "train" for m in missed)
    if where == "eval":  # a skipped draw at eval time moves every later draw: it shows in the dev batches AND in the train batches after them
        assert any(m[0] == "eval" for m in missed) and any(m[0] == "train" for m in missed)


def test_rows_and_per_sample_structure(env, tmp_path):
    from multihop_dense_retrieval_amd import mhop_arena, mhop_data
    meta, tok = env["meta"], env["tok"]
    sets, ar = datasets(env), arenas(env)
    for tag in ("eval", "train"):
        a, ds = ar[tag], sets[tag]
        row = lambda r: a.tokens[a.offsets[r]:a.offsets[r + 1]].tolist()  # noqa: E731
        comparison = np.array([s["type"] == "comparison" for s in ds.data])
        assert np.array_equal(a.start < 0, comparison)
        assert np.array_equal(a.qsp_rows[:, 1] >= 0, comparison) and (a.qsp_rows[:, 0] >= 0).all()  # two q_sp rows, or one
        n_neg = np.diff(a.neg_index)
        assert n_neg.tolist() == [len(s["neg_paras"]) for s in ds.data]
        assert a.n_rows == a.n + len(set(a.pos_rows.reshape(-1)) | set(a.neg_rows)) + int((a.qsp_rows >= 0).sum())
        assert a.n_rows < 6 * sum(1 for t, _ in meta["items"] if t == tag)  # fewer rows than sequences the reference's run tokenised
        for i, s in enumerate(ds.data):
            q = s["question"][:-1] if s["question"].endswith("?") else s["question"]
            assert row(a.q_row[i]) == mhop_data._single(tok, q, ds.max_q_len)["input_ids"].view(-1).tolist()
            for k in range(2):
                assert row(a.pos_rows[i, k]) == ds.encode_para(s["pos_paras"][k], ds.max_c_len)["input_ids"].view(-1).tolist()
            for k, neg in enumerate(s["neg_paras"]):
                assert row(a.neg_rows[a.neg_index[i] + k]) == ds.encode_para(neg, ds.max_c_len)["input_ids"].view(-1).tolist()
            starts = (0, 1) if comparison[i] else (int(a.start[i]),)
            if not comparison[i]:
                assert s["pos_paras"][starts[0]]["title"] != s["bridge"] and s["pos_paras"][1 - starts[0]]["title"] == s["bridge"]
            for slot, k in enumerate(starts):
                want = mhop_data._pair(tok, q, s["pos_paras"][k]["text"].strip(), ds.max_q_sp_len)["input_ids"].view(-1).tolist()
                assert row(a.qsp_rows[i, slot]) == want
        assert int(a.lens.max()) <= max(env["lens"]) and int(a.lens.min()) >= 2
    # the train branch's select(): the sample with one tfidf negative is dropped, the sample without the key keeps its neg_paras
    kept = [s for i, s in enumerate(meta["samples"]) if i != meta["dropped"]]
    keyless = kept.index(meta["samples"][meta["keyless"]])
    a = ar["train"]
    assert a.n == len(kept) == len(meta["samples"]) - 1
    assert [p["title"] for p in sets["train"].data[keyless]["neg_paras"]] == [p["title"] for p in meta["samples"][meta["keyless"]]["neg_paras"]]
    assert int(np.diff(a.neg_index)[keyless]) == len(meta["samples"][meta["keyless"]]["neg_paras"])
    # passages with one (title.strip(), text.strip()) share a row, within a sample and across samples
    one, two = json.loads(json.dumps(meta["samples"][1])), json.loads(json.dumps(meta["samples"][2]))
    two["tfidf_neg"][0] = dict(one["pos_paras"][0], title="  " + one["pos_paras"][0]["title"] + " ")
    two["tfidf_neg"][1] = dict(two["tfidf_neg"][2])
    shared = str(tmp_path / "shared.jsonl")
    with open(shared, "w") as f:
        f.write("\n".join(json.dumps(s) for s in (one, two)))
    a = mhop_arena.MhopArena.from_dataset(mhop_data.MhopTrainDataset(tok, shared, *env["lens"]))
    references = 2 * a.n + len(a.neg_rows)
    assert len(set(a.pos_rows.reshape(-1)) | set(a.neg_rows)) == references - 2
    assert a.neg_rows[a.neg_index[1]] == a.pos_rows[0, 0] and a.neg_rows[a.neg_index[1] + 1] == a.neg_rows[a.neg_index[1] + 2]
    assert a.n_rows == a.n + references - 2 + int((a.qsp_rows >= 0).sum())


def test_bad_index_arrays_are_refused():
    from multihop_dense_retrieval_amd.mhop_arena import MhopArena
    ok = dict(tokens=[0, 2, 0, 5, 2, 0, 6, 2, 0, 7, 2, 0, 8, 2, 0, 5, 2, 2, 6, 2], offsets=[0, 2, 5, 8, 11, 14, 20], q_row=[0], pos_rows=[[1, 2]],
              start=[1], qsp_rows=[[5, -1]], neg_index=[0, 2], neg_rows=[3, 4], train=True)
    a = MhopArena(**ok)
    assert a.n == 1 and a.n_rows == 6 and a.bytes_per_sample > 0
    table, widths = a.choose([0])
    assert table[0, :4].tolist() == [0, 5, 2, 1] and sorted(table[0, 4:].tolist()) == [3, 4] and widths == (2, 6, 3, 3, 3, 3)
    for key, bad in (("offsets", [0, 2, 5, 8, 11, 14, 21]), ("offsets", [0, 5, 2, 8, 11, 14, 20]), ("neg_index", [0, 1]), ("neg_index", [0, 3]),
                     ("neg_rows", [3, 6]), ("q_row", [-1]), ("pos_rows", [[1, 9]]), ("start", [2]), ("qsp_rows", [[-1, 5]]), ("start", [-1])):
        with pytest.raises(ValueError):
            MhopArena(**dict(ok, **{key: bad}))
    with pytest.raises(IndexError):
        a.choose([1])
    assert a.widths(np.array([[-1, 6, 11, 0, 0, 0]])) == (1, 1, 1, 2, 2, 2)  # rows outside the arena are empty


def test_cache_round_trip_rebuilds_and_refusals(env, tmp_path, capsys, monkeypatch):
    from multihop_dense_retrieval_amd import mhop_arena, mhop_data
    A, tok, lens = mhop_arena.MhopArena, env["tok"], env["lens"]
    train_file = str(tmp_path / "train.jsonl")
    with open(train_file, "wb") as f:
        f.write(open(env["files"]["train"], "rb").read())
    ds = mhop_data.MhopTrainDataset(tok, train_file, *lens)
    arena = A.from_dataset(ds)
    tag = mhop_arena.mhop_arena_tag(tok, *lens, True, train_file)
    path = str(tmp_path / "a.npz")
    arena.save(path, tag=tag)
    back = A.load(path, expect_tag=tag)
    assert back.train and back.n == arena.n and back.n_rows == arena.n_rows
    for name, _ in mhop_arena._ARRAYS:
        x, y = getattr(arena, name), getattr(back, name)
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    others = [mhop_arena.mhop_arena_tag(tok, lens[0] + 1, lens[1], lens[2], True, train_file), mhop_arena.mhop_arena_tag(tok, lens[0], lens[1] - 1, lens[2], True, train_file),
              mhop_arena.mhop_arena_tag(tok, lens[0], lens[1], lens[2] + 1, True, train_file), mhop_arena.mhop_arena_tag(tok, *lens, False, train_file),
              "qa-train-arena-v1|something else", ""]
    for other in others:
        assert other != tag and A.load(path, expect_tag=other) is None
    st = os.stat(train_file)
    os.utime(train_file, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))  # another mtime: another tag
    assert mhop_arena.mhop_arena_tag(tok, *lens, True, train_file) != tag
    os.utime(train_file, ns=(st.st_atime_ns, st.st_mtime_ns))
    assert mhop_arena.mhop_arena_tag(tok, *lens, True, train_file) == tag
    with open(train_file, "ab") as f:  # another size: another tag
        f.write(b"\n")
    assert mhop_arena.mhop_arena_tag(tok, *lens, True, train_file) != tag

    # load_or_build: builds and writes the cache beside the data file, then reads it back, and says which on stdout
    cache = train_file + ".mhop_arena.npz"
    capsys.readouterr()
    one = A.load_or_build(train_file, ds, tok)
    said = capsys.readouterr().out
    assert "Tokenising" in said and "Loaded" not in said and os.path.exists(cache)
    two = A.load_or_build(train_file, ds, tok)
    said = capsys.readouterr().out
    assert "Loaded the token arena" in said and "Tokenising" not in said and np.array_equal(one.tokens, two.tokens) and two.train
    assert sorted(os.listdir(tmp_path)) == ["a.npz", "train.jsonl", "train.jsonl.mhop_arena.npz"]  # no temporary file is left
    # another cut, another branch, another file size: a rebuild, and the cache is the new one's afterwards
    shorter = mhop_data.MhopTrainDataset(tok, train_file, lens[0], lens[1], lens[2] - 5)
    capsys.readouterr()
    three = A.load_or_build(train_file, shorter, tok)
    assert "Tokenising" in capsys.readouterr().out and int(three.lens.max()) < int(one.lens.max())
    assert A.load(cache, expect_tag=mhop_arena.mhop_arena_tag(tok, lens[0], lens[1], lens[2] - 5, True, train_file)) is not None
    as_eval = mhop_data.MhopDataset(tok, train_file, lens[0], lens[1], lens[2] - 5)
    four = A.load_or_build(train_file, as_eval, tok)
    assert "Tokenising" in capsys.readouterr().out and not four.train and four.n == as_eval.__len__() == three.n + 1
    with open(train_file, "ab") as f:
        f.write(b"\n")
    A.load_or_build(train_file, as_eval, tok)
    assert "Tokenising" in capsys.readouterr().out
    A.load_or_build(train_file, as_eval, tok)
    assert "Loaded" in capsys.readouterr().out
    # a foreign file under the cache's name is never reused
    np.savez(cache, tag=np.array("arena-v2|someone else's"), tokens=np.zeros(3, np.int32))
    five = A.load_or_build(train_file, as_eval, tok)
    assert "Tokenising" in capsys.readouterr().out and np.array_equal(five.tokens, four.tokens)

    # an unwritable directory: the arena is built, nothing is saved, and stdout says so
    locked = tmp_path / "locked"
    locked.mkdir()
    data_file = str(locked / "dev.jsonl")
    with open(data_file, "wb") as f:
        f.write(open(env["files"]["eval"], "rb").read())
    dev = mhop_data.MhopDataset(tok, data_file, *lens)
    os.chmod(locked, 0o555)
    try:
        if os.access(str(locked), os.W_OK):  # a superuser writes there anyway: the same refusal from the write itself
            def refuse(*a, **k):
                raise PermissionError(13, "Permission denied")
            monkeypatch.setattr(mhop_arena.np, "savez", refuse)
        capsys.readouterr()
        six = A.load_or_build(data_file, dev, tok)
        said = capsys.readouterr().out
        assert six.n == 24 and "not cached" in said and os.listdir(locked) == ["dev.jsonl"]
    finally:
        monkeypatch.undo()
        os.chmod(locked, 0o755)


def test_other_tokenizer_families_are_refused_with_a_message(env):
    import transformers
    from multihop_dense_retrieval_amd import mhop_arena, mhop_data
    bert = transformers.BertTokenizer(os.path.join(GOLD, "reader_electra_tiny", "vocab.txt"), do_lower_case=True)
    ds = mhop_data.MhopDataset(bert, env["files"]["eval"], *env["lens"])
    for call in (lambda: mhop_arena.MhopArena.from_dataset(ds), lambda: mhop_arena.MhopArena.load_or_build(env["files"]["eval"], ds, bert)):
        with pytest.raises(TypeError, match="RoBERTa-family tokenizers only.*BertTokenizer"):
            call()
    assert not os.path.exists(env["files"]["eval"] + ".mhop_arena.npz")


def test_header_binding_and_library_agree():
    """include/mdr_mhop_train.h declares exactly what mhop_arena.SIGNATURES binds and the library exports, apart from every other header's
    table; the signature has the prototype's number of arguments; the struct's fields are the header's; the native source reads no
    environment variable."""
    import importlib
    from multihop_dense_retrieval_amd import _lib, build, mhop_arena
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdr_mhop_train.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(mhop_arena.SIGNATURES) == sorted(mhop_arena.EXPORTED_SYMBOLS) == ["mdr_mhop_assemble"]
    assert not set(declared) & set(_lib.EXPORTED_SYMBOLS)
    for mod, attr in (("attention", "SIGNATURES"), ("linear", "SIGNATURES"), ("layernorm", "SIGNATURES"), ("embedding", "SIGNATURES"), ("optim", "SIGNATURES"),
                      ("criterions", "SIGNATURES"), ("criterions", "LOSS_SIGNATURES"), ("reader", "SIGNATURES"), ("qa_train_arena", "SIGNATURES"),
                      ("momentum", "SIGNATURES")):
        assert not set(declared) & set(getattr(importlib.import_module("multihop_dense_retrieval_amd." + mod), attr)), mod
    for name, (_, args) in mhop_arena.SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args) == proto.count(",") + 1, name
    lib = ctypes.CDLL(build.build_lib())
    assert hasattr(lib, "mdr_mhop_assemble")
    mhop_arena.lib()
    src = open(os.path.join(ROOT, "multihop_dense_retrieval_amd", "csrc", "mdr_mhop_train.hip")).read()
    assert "getenv" not in src
    body = re.search(r"typedef struct mdr_mhop_arena \{(.*?)\} mdr_mhop_arena;", text, flags=re.S).group(1)
    assert re.findall(r"\b(\w+);", body) == [f[0] for f in mhop_arena.Arena._fields_]
    assert int(re.search(r"#define MDR_MHOP_SLOTS (\d+)", text).group(1)) == len(mhop_arena.SLOTS) == 6
