"""CPU: the reader's evaluation pieces and the chain-selection rule (multihop_dense_retrieval_amd/qa_eval.py).

Rows: QAEvalPieces.assemble_host equals qa_collate of the QADataset items on both fixtures, at three batch sizes and at max_seq_len values
that cut rows inside P1 and inside P2, widths, sent_offsets and para_offsets included; the arrays do not depend on the worker count; the
cache round-trips and a foreign tag rebuilds it. Rule: select_host (the kernel's rule in numpy) equals select_sweep_host (predict()'s
literal list.sort calls) on a tie-heavy and a low-tie family, with one factor and with sixteen, and the tie-heavy family tells the rule
from "first chain with the largest key". Host halves: fed the same fabricated head outputs -- a question with NaN, +inf and -inf among
them -- the host path (qa_data.chain_results + predict_metrics / final_results) and the arena path (ScoreTable + qa_eval.predict_metrics /
final_results) log the same lines and return the same objects. The refusals; check_offsets; include/mdr_reader_select.h, the binding table
and the library agree. (The kernel: tests/test_reader_select_gpu.py.)"""
import ctypes
import json
import logging
import os
import re
import sys
from functools import partial

import numpy as np
import pytest
import torch

import select_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")
# (file, max_seq_len of its golden run, max_q_len, two max_seq_len that cut rows: the first inside P1, the second inside P2)
FIXTURES = {"reader": (os.path.join(ASSETS, "items.jsonl"), 160, 24, (40, 60), (5, 15, 30)),
            "train": (os.path.join(GOLD, "qa_train_items.jsonl"), 48, 24, (20, 30), (9, 29, 48))}


@pytest.fixture(scope="module")
def tok():
    import transformers
    return transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)


def host_batches(tok, path, max_seq_len, max_q_len, batch_size):
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import qa_data
    ds = qa_data.QADataset(tok, path, max_seq_len, max_q_len)
    return list(DataLoader(ds, batch_size=batch_size, collate_fn=partial(qa_data.qa_collate, pad_id=tok.pad_token_id)))


def assert_rows_equal(rows, batch, where):
    """rows: QAEvalPieces.assemble_host / assemble (as numpy) of the batch's items; batch: qa_collate's."""
    net = batch["net_inputs"]
    for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets", "label"):
        want = net[k].to(torch.int64).numpy()  # (qa_collate's paragraph_mask is float 0 / 1)
        assert rows[k].dtype == np.int64 and rows[k].shape == want.shape and np.array_equal(rows[k], want), (where, k)
    assert rows["para_offsets"].tolist() == batch["para_offsets"], where
    assert rows["lengths"].tolist() == net["attention_mask"].sum(1).tolist(), where


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_rows_equal_qa_collate(tok, name):
    from multihop_dense_retrieval_amd import qa_data, qa_eval
    path, full, max_q_len, cuts, counts = FIXTURES[name]
    records, seg = qa_eval.read_eval_file(path)
    assert records == qa_data.QADataset(tok, path, full, max_q_len).data  # the file as QADataset(train=False) reads it
    in_p1 = in_p2 = 0
    for max_seq_len in (full,) + cuts:
        for bs in (1, 4, 64):
            pieces = qa_eval.QAEvalPieces.from_file(path, tok, max_seq_len, max_q_len, bs)
            assert (pieces.n_questions, pieces.n, pieces.n_passages) == counts
            batches = host_batches(tok, path, max_seq_len, max_q_len, bs)
            assert len(batches) == len(pieces.batches)
            for (lo, hi), b in zip(pieces.batches, batches):
                assert_rows_equal(pieces.assemble_host(lo, hi), b, (max_seq_len, bs, lo))
                assert pieces.batch_shape(lo, hi) == (b["net_inputs"]["input_ids"].shape[1], b["net_inputs"]["sent_offsets"].shape[1])
        if max_seq_len != full:
            l0, l1 = (pieces.passages.lens[pieces.items[:, c]] for c in (1, 2))
            n_wp = pieces.lens - pieces.para_offset - 1
            in_p1 += int(((n_wp > 3) & (n_wp < 3 + l0)).sum())
            in_p2 += int(((n_wp > 4 + l0) & (n_wp < 4 + l0 + l1)).sum())
    assert in_p1 and in_p2  # the cuts cut where they claim to
    assert len(pieces.qids) == counts[0] and list(pieces.gold) == pieces.qids


def test_arrays_do_not_depend_on_the_worker_count(tok):
    from multihop_dense_retrieval_amd import qa_eval
    path, full, max_q_len, _, _ = FIXTURES["train"]
    one, many = (qa_eval.QAEvalPieces.from_file(path, tok, full, max_q_len, 8, workers=w) for w in (0, 3))
    for n, _ in qa_eval._ARRAYS:
        a, b = getattr(one, n), getattr(many, n)
        assert a.dtype == b.dtype and np.array_equal(a, b), n


def test_cache_round_trips_and_a_foreign_tag_rebuilds(tok, tmp_path):
    from multihop_dense_retrieval_amd import qa_eval
    src, full, max_q_len, _, _ = FIXTURES["train"]
    path = str(tmp_path / "dev.jsonl")
    with open(path, "wb") as f:
        f.write(open(src, "rb").read())
    said = []
    build = lambda q_len=max_q_len: qa_eval.QAEvalPieces.load_or_build(path, tok, full, q_len, 8, log=said.append)  # noqa: E731
    first = build()
    cache = path + ".qa_eval_pieces.npz"
    assert os.path.exists(cache) and said[-1].startswith("Preparing the dev set once") and sorted(os.listdir(tmp_path)) == ["dev.jsonl", "dev.jsonl.qa_eval_pieces.npz"]
    second = build()
    assert said[-1].startswith("Loaded the reader's evaluation pieces from")
    for n, _ in qa_eval._ARRAYS:
        assert np.array_equal(getattr(first, n), getattr(second, n)) and getattr(first, n).dtype == getattr(second, n).dtype, n
    assert str(np.load(cache)["tag"]) == qa_eval.eval_pieces_tag(tok, max_q_len, path)
    tag = qa_eval.eval_pieces_tag(tok, max_q_len, path)
    assert tag.startswith(qa_eval.RULE + "|qa-arena-v1|") and f"|max_q_len={max_q_len}|file=" in tag
    build(q_len=3)  # another max_q_len: a foreign tag
    assert said[-1].startswith("Preparing the dev set once")
    z = dict(np.load(cache))
    z["tag"] = np.array("qa-eval-pieces-v0|something else")
    np.savez(cache, **z)
    build(q_len=3)
    assert said[-1].startswith("Preparing the dev set once") and str(np.load(cache)["tag"]) == qa_eval.eval_pieces_tag(tok, 3, path)


# ---- the selection rule ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", ["tie_heavy", "low_tie"])
@pytest.mark.parametrize("lambdas", [cases.SWEEP, [0.8], cases.SIXTEEN], ids=["sweep", "one", "sixteen"])
def test_select_host_equals_the_literal_sorts(family, lambdas):
    from multihop_dense_retrieval_amd import qa_eval
    rank, span, q = getattr(cases, family)(11, 4000 if lambdas is cases.SWEEP else 600)
    sizes = np.diff(q)
    assert set(cases.BASE_SIZES + cases.EDGE_SIZES) == set(sizes.tolist())
    want_w, want_r = qa_eval.select_sweep_host(rank, span, q, lambdas)
    got_w, got_r, flags = qa_eval.select_host(rank, span, q, lambdas)
    assert not flags.any() and got_w.dtype == got_r.dtype == np.int32
    assert np.array_equal(got_r, want_r) and np.array_equal(got_w, want_w)
    assert (got_w[sizes == 0] == -1).all() and (got_r[sizes == 0] == -1).all() and (got_w[sizes > 0] >= 0).all()
    assert ((got_w >= q[:-1, None]) & (got_w < q[1:, None]))[sizes > 0].all()  # item indices, inside the question
    # the bit patterns are as good as the floats
    again = qa_eval.select_host(rank.view(np.int16), span.view(np.uint16), q, lambdas)
    assert np.array_equal(again[0], got_w)
    if family == "tie_heavy" and lambdas is cases.SWEEP:
        first = qa_eval.select_host(rank, span, q, lambdas, first_index=True)[0]
        differ = int((first != want_w).sum())
        print(f"[select] first-index rule differs from the literal sorts in {differ} of {want_w.size} (question, factor) pairs")
        assert differ >= 1  # these inputs tell the two rules apart
    if len(lambdas) == 1:  # sorted once from file order: the two rules coincide
        assert np.array_equal(qa_eval.select_host(rank, span, q, lambdas, first_index=True)[0], want_w)


def test_select_host_flags_non_finite_scores():
    from multihop_dense_retrieval_amd import qa_eval
    rank, span, q = cases.low_tie(5, 40, edge_repeats=1)
    want = qa_eval.select_sweep_host(rank, span, q, cases.SWEEP)
    big = [j for j in range(40) if q[j + 1] - q[j] >= 2][:3]
    rank[q[big[0]]], span[q[big[1] + 1] - 1], rank[q[big[2]] + 1] = np.nan, np.inf, -np.inf
    w, r, flags = qa_eval.select_host(rank, span, q, cases.SWEEP)
    assert sorted(np.nonzero(flags)[0].tolist()) == sorted(big)
    assert (w[big] == -1).all() and (r[big] == -1).all()
    rest = np.setdiff1d(np.arange(40), big)
    assert np.array_equal(w[rest], want[0][rest]) and np.array_equal(r[rest], want[1][rest])


def test_check_offsets_states_the_kernels_contract():
    from multihop_dense_retrieval_amd import qa_eval
    ok = np.array([0, 0, 3, 3, 7], np.int64)
    assert qa_eval.check_offsets(ok, 7) is not None and qa_eval.check_offsets(np.array([2, 5], np.int64), 9) is not None
    for bad, n in ((np.array([-1, 2], np.int64), 5), (np.array([0, 4, 3, 7], np.int64), 7), (ok, 6), (ok.astype(np.int32), 7), (ok.reshape(1, -1), 7),
                   (np.zeros(0, np.int64), 0), (np.array([0, 2 ** 31], np.int64), 2 ** 31)):
        with pytest.raises(ValueError):
            qa_eval.check_offsets(bad, n)


# ---- the two paths' host halves on fabricated head outputs ------------------------------------------------------------------------------


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def logged(name, fn):
    logger = logging.getLogger(name)
    logger.setLevel(logging.INFO)
    logger.propagate = False
    h = _Lines()
    logger.addHandler(h)
    try:
        return fn(logger), h.lines
    finally:
        logger.removeHandler(h)


def fabricated_heads(batches, seed, bad_items):
    """Per batch decode()'s dict, fp16-exact: scores on a coarse grid (ties), spans inside the row's paragraph, sp_prob fp16 on
    [R, S_b]; bad_items: {item: (rank, span)} planted verbatim."""
    rng = np.random.default_rng(seed)
    grid = np.arange(-2, 2.5, 0.5).astype(np.float16)
    heads, i0 = [], 0
    for b in batches:
        R, S = b["net_inputs"]["input_ids"].shape[0], b["net_inputs"]["sent_offsets"].shape[1]
        rel = [int(rng.integers(0, len(wp))) for wp in b["wp_tokens"]]
        end = [min(len(wp) - 1, s + int(rng.integers(0, 4))) for s, wp in zip(rel, b["wp_tokens"])]
        rank, span = rng.choice(grid, R), rng.choice(grid, R)
        for i, (r, s) in bad_items.items():
            if i0 <= i < i0 + R:
                rank[i - i0], span[i - i0] = r, s
        heads.append({"start": torch.tensor([s + po for s, po in zip(rel, b["para_offsets"])]), "end": torch.tensor([e + po for e, po in zip(end, b["para_offsets"])]),
                      "span_score": torch.from_numpy(span), "rank_score": torch.from_numpy(rank).reshape(R, 1),
                      "sp_prob": torch.from_numpy(rng.choice(np.arange(0, 1.01, 0.125), (R, S)).astype(np.float16))})
        i0 += R
    return heads


def host_chains(batches, heads, sp_pred, final):
    """scripts/train_qa.py run_batches, from given head outputs."""
    from multihop_dense_retrieval_amd import qa_data
    chains, gold = [], {}
    for b, head in zip(batches, heads):
        lists = {"start": head["start"].tolist(), "end": head["end"].tolist(), "span_score": head["span_score"].float().tolist(),
                 "rank_score": head["rank_score"].view(-1).float().tolist(), "sp_prob": head["sp_prob"].float().tolist() if sp_pred else None}
        chains.extend(qa_data.chain_results(b, lists, sp_pred, final=final))
        for idx, qid in enumerate(b["qids"]):
            gold[qid] = (b["gold_answer"][idx], b["sp_gold"][idx])
    return chains, gold


@pytest.mark.parametrize("name,bs", [("reader", 4), ("train", 8), ("train", 3)])
@pytest.mark.parametrize("sp_pred", [True, False], ids=["sp", "nosp"])
def test_host_halves_agree_on_fabricated_head_outputs(tok, name, bs, sp_pred):
    from multihop_dense_retrieval_amd import qa_data, qa_eval
    path, full, max_q_len, _, _ = FIXTURES[name]
    pieces = qa_eval.QAEvalPieces.from_file(path, tok, full, max_q_len, bs)
    batches = host_batches(tok, path, full, max_q_len, bs)
    seg = pieces.seg_offsets
    j = int(np.argmax(np.diff(seg) >= 3))  # a question of three chains or more: NaN, +inf and -inf in it
    lo = int(seg[j])
    bad = {lo: (np.nan, 0.5), lo + 1: (np.inf, -np.inf), lo + 2: (-np.inf, 1.0)}
    heads = fabricated_heads(batches, 7, bad)
    table = qa_eval.ScoreTable(pieces.n, pieces.max_sents, "cpu")
    for (b_lo, _), head in zip(pieces.batches, heads):
        table.put(b_lo, head if sp_pred else {**head, "sp_prob": None})
    assert table.batch_sents == [h["sp_prob"].shape[1] if sp_pred else 0 for h in heads]
    for fixed in (None, 0.8):
        chains, gold = host_chains(batches, heads, sp_pred, final=False)
        (want, want_best), want_lines = logged("qa-eval-host", lambda lg: qa_data.predict_metrics(chains, gold, sp_pred, lg, fixed_thresh=fixed))
        (got, got_best), got_lines = logged("qa-eval-arena", lambda lg: qa_eval.predict_metrics(pieces, table, tok, sp_pred, lg, fixed_thresh=fixed, host=True))
        assert got_lines == want_lines and len(want_lines) == 3 + 7 * (11 if fixed is None else 1)
        assert json.dumps(got) == json.dumps(want) and list(got) == list(want)
        assert json.dumps(got_best) == json.dumps(want_best)
        assert (want_best is None) == (not sp_pred or want["joint_f1"] == 0)
    chains, _ = host_chains(batches, heads, sp_pred, final=True)
    assert json.dumps(qa_eval.final_results(pieces, table, tok, sp_pred, host=True)) == json.dumps(qa_data.final_results(chains, weight=0.8))
    w = qa_eval.Winners(pieces, table, cases.SWEEP, tok, sp_pred, final=False, host=True)
    assert w.flagged == 1 and (w.winners[j] >= lo).all() and w.distinct == len(w.answers) <= pieces.n_questions * 11
    assert w.distinct < pieces.n  # fewer decodes than chains: what the arena path is for


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------


def load_script(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_refusals_name_the_host_path_and_leave_no_cache(tok, tmp_path):
    from multihop_dense_retrieval_amd import qa_eval
    lines = [json.loads(ln) for ln in open(FIXTURES["train"][0])]
    three = json.loads(json.dumps(lines))
    three[2]["candidate_chains"][0] = three[2]["candidate_chains"][0] + three[2]["candidate_chains"][0][:1]
    twice = json.loads(json.dumps(lines))
    twice[4]["_id"] = twice[1]["_id"]
    script = load_script("train_qa")
    for name, data, word in (("three", three, "a chain of 3 passages"), ("twice", twice, "repeats the _id")):
        path = str(tmp_path / f"{name}.jsonl")
        with open(path, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in data))
        with pytest.raises(ValueError, match=word):
            qa_eval.read_eval_file(path)
        args = script.train_args(["--eval-arena", "--predict_file", path, "--max_seq_len", "48", "--max_q_len", "24", "--num_workers", "0"])
        assert args.eval_arena and not script.train_args([]).eval_arena
        with pytest.raises(SystemExit) as e:
            script.eval_pieces_for(args, tok, logging.getLogger("refusals"))
        assert str(e.value).startswith("--eval-arena is not supported: ") and word in str(e.value) and "run without --eval-arena" in str(e.value)
        assert sorted(os.listdir(tmp_path)) == sorted(p for p in os.listdir(tmp_path) if p.endswith(".jsonl"))  # no cache, no temporary file

    class NoYes:
        cls_token, sep_token, pad_token_id = "[CLS]", "[SEP]", 0

        def tokenize(self, text):
            return ["y", "##es"] if text == "yes" else tok.tokenize(text)

        def __getattr__(self, name):
            return getattr(tok, name)

    good = str(tmp_path / "good.jsonl")
    with open(good, "w") as f:
        f.write("".join(json.dumps(x) + "\n" for x in lines))
    args = script.train_args(["--eval-arena", "--predict_file", good, "--max_seq_len", "48", "--max_q_len", "24", "--num_workers", "0"])
    with pytest.raises(SystemExit) as e:
        script.eval_pieces_for(args, NoYes(), logging.getLogger("refusals"))
    assert str(e.value).startswith("--eval-arena is not supported: 'yes' is not a single WordPiece")
    assert not [p for p in os.listdir(tmp_path) if not p.endswith(".jsonl")]
    args.max_seq_len = 14  # the longest question has 9 WordPieces: no room for yes no [SEP]
    with pytest.raises(SystemExit) as e:
        script.eval_pieces_for(args, tok, logging.getLogger("refusals"))
    assert "leaves no room" in str(e.value)


# ---- header, binding, library ------------------------------------------------------------------------------------------------------------


def test_header_binding_and_library_agree():
    """include/mdr_reader_select.h declares exactly what qa_eval.SIGNATURES binds and the library exports, apart from every other header's
    table (include/mdr_reader.h's and include/mdr_hip.h's among them); the signature has the prototype's arguments; the limit is the
    header's; the native source reads no environment variable and holds no atomics."""
    import importlib
    from multihop_dense_retrieval_amd import _lib, build, qa_eval, qa_train_arena, qa_train_pieces
    raw = open(os.path.join(ROOT, "include", "mdr_reader_select.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(qa_eval.SIGNATURES) == sorted(qa_eval.EXPORTED_SYMBOLS) == ["mdr_reader_select"]
    assert not set(declared) & set(_lib.EXPORTED_SYMBOLS) and not set(declared) & set(qa_train_arena.SIGNATURES) and not set(declared) & set(qa_train_pieces.SIGNATURES)
    for mod, attr in (("attention", "SIGNATURES"), ("linear", "SIGNATURES"), ("layernorm", "SIGNATURES"), ("embedding", "SIGNATURES"), ("optim", "SIGNATURES"),
                      ("criterions", "SIGNATURES"), ("criterions", "LOSS_SIGNATURES"), ("reader", "SIGNATURES")):
        assert not set(declared) & set(getattr(importlib.import_module("multihop_dense_retrieval_amd." + mod), attr)), mod
    for header in ("mdr_reader.h", "mdr_hip.h"):
        assert "mdr_reader_select" not in open(os.path.join(ROOT, "include", header)).read(), header
    (_, args), = qa_eval.SIGNATURES.values()
    proto = [a.strip() for a in re.search(r"\bmdr_reader_select\s*\(([^)]*)\)", text).group(1).split(",")]
    assert len(args) == len(proto) == 12 and proto[-2:] == ["int device", "void* stream"]
    assert [a.split()[-1] for a in proto[:10]] == ["rank16_dev", "span16_dev", "q_offsets_dev", "n_q", "lambdas", "one_minus", "n_lambda", "winners_dev",
                                                  "rank_top_dev", "flags_dev"]
    assert int(re.search(r"#define MDR_READER_SELECT_MAX_LAMBDAS (\d+)", text).group(1)) == qa_eval.MAX_LAMBDAS == 16
    lib = ctypes.CDLL(build.build_lib())
    assert hasattr(lib, "mdr_reader_select")
    qa_eval.lib()
    src = open(os.path.join(ROOT, "multihop_dense_retrieval_amd", "csrc", "mdr_reader_select.hip")).read()
    assert "getenv" not in src and not re.search(r"atomic\w*\s*\(", src, flags=re.I) and "#pragma clang fp contract(off)" in src
    assert not re.search(r"hipMalloc|hipMemcpy|Synchronize", src)  # the launcher copies, allocates and waits for nothing
