"""GPU (-m gpu): mdr_reader_train_assemble (include/mdr_reader_train.h) against QATrainArena.assemble_host, bit for bit: on the fixture arena
for every batch of the golden's first epoch, and on a random arena (item lengths 0 to 48, 0 to 6 sentences, 1 to 4 spans, plus ONE item of
300 tokens so that the token copy itself, not only the padding, goes past one pass of the 256 threads) over the grid rows {1, 3, 7} x
out_len {1, 24, 48, 257, 300} x n_sent {0, 1, 5} x n_span {1, 3}. Every output sits between guard rows (tests/guarded.py)."""
import json
import os

import numpy as np
import pytest
import torch

from guarded import Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ITEMS = os.path.join(GOLD, "qa_train_items.jsonl")
KEYS2 = ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask")
LONG = 12  # the random arena's 300-token item


def shapes_of(R, L, S, P):
    return {**{k: (R, L) for k in KEYS2}, "sent_offsets": (R, S), "sent_labels": (R, S), "starts": (R, P), "ends": (R, P), "label": (R, 1),
            "ans_covered": (R, 1), "para_offsets": (R,), "lengths": (R,)}


def guarded_call(arena, idx, L, S, P, pad_id):
    """assemble into guarded buffers; returns {key: numpy} having checked that nothing outside the call's rows was written"""
    R = len(idx)
    bufs = {k: Guarded(R, s[1:], torch.int64, 2, 3, name=k) for k, s in shapes_of(R, L, S, P).items()}
    out = arena.assemble(torch.tensor(idx, dtype=torch.int64, device="cuda"), L, S, P, pad_id, out={k: g.own for k, g in bufs.items()})
    torch.cuda.synchronize()
    assert all(out[k].data_ptr() == bufs[k].own.data_ptr() for k in bufs)
    return {k: g.checked() for k, g in bufs.items()}


def assert_same(got, want, where):
    for k, w in want.items():
        assert got[k].shape == w.shape and got[k].dtype == np.int64 and np.array_equal(got[k], w), (where, k)


@pytest.fixture(scope="module")
def fixture_arena():
    import transformers
    from multihop_dense_retrieval_amd import qa_train_arena, qa_train_data
    meta = json.load(open(os.path.join(GOLD, "qa_train_ref.json")))
    tok = transformers.BertTokenizer(os.path.join(GOLD, "reader_electra_tiny", "vocab.txt"), do_lower_case=True)
    ds = qa_train_data.QATrainDataset(tok, ITEMS, meta["max_seq_len"], meta["max_q_len"])
    return qa_train_arena.QATrainArena.from_dataset(ds).to("cuda"), meta, tok


@pytest.fixture(scope="module")
def random_arena():
    from multihop_dense_retrieval_amd import qa_train_arena
    rng = np.random.default_rng(11)
    lens = list(rng.integers(0, 49, 12)) + [300]
    lens[3], lens[5] = 0, 48
    ns = list(rng.integers(0, 7, 13))
    nsp = list(rng.integers(1, 5, 13))
    ns[0], ns[1], nsp[0], nsp[1] = 0, 6, 1, 4
    po = [int(rng.integers(0, n + 1)) for n in lens]
    tokens = rng.integers(1, 500, int(np.sum(lens))).astype(np.int32)
    cum = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int64)  # noqa: E731
    arena = qa_train_arena.QATrainArena(tokens, cum(lens), po, rng.integers(1, 300, int(np.sum(ns))), rng.integers(0, 2, int(np.sum(ns))), cum(ns),
                                        rng.integers(-1, 300, (int(np.sum(nsp)), 2)), cum(nsp), rng.integers(0, 2, 13), rng.integers(0, 2, 13))
    assert arena.n == 13 and arena.lens[LONG] == 300
    return arena.to("cuda")


def test_fixture_batches_equal_the_host_assembly_and_the_reference(fixture_arena):
    arena, meta, tok = fixture_arena
    z = np.load(os.path.join(GOLD, "qa_train_ref.npz"))
    first = meta["epochs"][0]
    for bi, lo in enumerate(range(0, len(first), meta["batch"])):
        idx = first[lo:lo + meta["batch"]]
        L, S, P = arena.batch_shape(idx)
        got = guarded_call(arena, idx, L, S, P, tok.pad_token_id)
        assert_same(got, arena.assemble_host(idx, pad_id=tok.pad_token_id), f"batch {bi}")
        for k in (k.split(".", 1)[1] for k in z.files if k.startswith(f"b{bi}.")):
            assert np.array_equal(got[k], z[f"b{bi}.{k}"]), (bi, k)  # the reference's qa_collate itself


def indices_for(rows, out_len, n):
    rng = np.random.default_rng(rows * 1000 + out_len)
    i, j, k = (int(x) for x in rng.integers(0, n - 1, 3))
    if rows == 1:
        return [LONG if out_len >= 257 else i]
    if rows == 3:
        return [-1, LONG if out_len >= 257 else i, n]
    return [i, i, -1, j, n, LONG, k]  # a repeated index, both sides outside the arena, the long item


@pytest.mark.parametrize("out_len", [1, 24, 48, 257, 300])
@pytest.mark.parametrize("rows", [1, 3, 7])
def test_random_arena_grid(random_arena, rows, out_len):
    arena = random_arena
    idx = indices_for(rows, out_len, arena.n)
    for n_sent in (0, 1, 5):
        for n_span in (1, 3):
            want = arena.assemble_host(idx, out_len, n_sent, n_span, pad_id=7)
            got = guarded_call(arena, idx, out_len, n_sent, n_span, 7)
            assert_same(got, want, (idx, n_sent, n_span))
            again = guarded_call(arena, idx, out_len, n_sent, n_span, 7)
            assert all(got[k].tobytes() == again[k].tobytes() for k in got), "two runs differ"
    # the cases this grid is for, on the last call: rows, sentences and spans longer than the widths are cut; rows outside are empty
    lens, ns, nsp = arena.lens[[i for i in idx if 0 <= i < arena.n]], arena.n_sents, arena.n_spans
    if rows == 7:
        assert lens.max() == 300 and (out_len < 300) == bool((want["lengths"] > out_len).any())
        assert ns[idx[0]] >= 0 and nsp.max() > 3 and ns.max() > 5
        for r in (2, 4):
            assert (got["input_ids"][r] == 7).all() and got["label"][r, 0] == -1 and (got["starts"][r] == -1).all() and got["lengths"][r] == 0
        assert np.array_equal(got["input_ids"][0], got["input_ids"][1])


def test_bad_arguments_are_refused(random_arena):
    arena = random_arena
    idx = torch.zeros(2, dtype=torch.int64, device="cuda")
    for bad in ((0, 1, 1), (8, -1, 1), (8, 1, 0)):
        with pytest.raises(ValueError):
            arena.assemble(idx, *bad)
    with pytest.raises(ValueError):
        arena.assemble(idx.to(torch.int32), 8, 1, 1)
    with pytest.raises(ValueError):
        arena.assemble(idx.cpu(), 8, 1, 1)
    empty = arena.assemble(idx[:0], 8, 1, 1)
    assert empty["input_ids"].shape == (0, 8) and empty["label"].shape == (0, 1)
