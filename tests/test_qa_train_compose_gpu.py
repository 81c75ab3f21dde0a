"""GPU (-m gpu): mdr_reader_train_compose (include/mdr_reader_train_pieces.h) against QATrainPieces.compose_host, bit for bit.

1  the fixture (tests/golden/qa_train_items.jsonl): every batch of the golden's first epoch equals compose_host and hence the reference's
   qa_collate (tests/golden/qa_train_ref.npz);
2  random piece arenas given as integer arrays (no tokenizer) over the grid rows {1, 3, 7} x out_len {1, 24, 48, 257, 300} x n_sent
   {0, 1, 5} x n_span {1, 3}, each at six values of max_seq_len chosen so that the TARGET row of the batch is cut right after yes no [SEP],
   inside P1, on the separator behind P1, on P2's first token, inside P2, and nowhere. The target of out_len >= 257 has a P1 of 600
   tokens (P1 alone passes the cut, and a thread walks its stride more than once); the arena also holds passages of 0 tokens and of 0
   sentences, questions of 0 tokens and of the stored maximum, items without labels and without pairs, an item whose pairs all lie in
   P2, pairs that straddle cuts, more pairs and sentences than the widths, and the batches hold the indices -1 and N.
   test_the_grid_holds_its_cases asserts on the expected outputs that each of these really occurs;
3  on the fixture, QATrainPieces.assemble and QATrainArena.assemble (mdr_reader_train_assemble) give equal tensors.
Every output sits between guard rows (tests/guarded.py); every launch is repeated and gives the same bytes."""
import functools
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
ROWS, OUT_LENS, N_SENTS, N_SPANS = (1, 3, 7), (1, 24, 48, 257, 300), (0, 1, 5), (1, 3)
CUTS = ("after yes no [SEP]", "inside P1", "on the separator behind P1", "on P2's first token", "inside P2", "nowhere")
SPECIAL = (901, 902, 903, 904)  # cls, sep, yes, no: outside the random token range
Q_MAX = 10    # the stored maximum of the question lengths
SMALL, BIG = 0, 1  # the target items: P1 of 9 tokens, P1 of 600 tokens
ALL_IN_P2 = 2      # an item whose pairs all start in P2


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


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def fixture_arenas():
    import transformers
    from multihop_dense_retrieval_amd import qa_train_arena, qa_train_data, qa_train_pieces
    meta = json.load(open(os.path.join(GOLD, "qa_train_ref.json")))
    tok = transformers.BertTokenizer(os.path.join(GOLD, "reader_electra_tiny", "vocab.txt"), do_lower_case=True)
    ds = qa_train_data.QATrainDataset(tok, ITEMS, meta["max_seq_len"], meta["max_q_len"])
    return qa_train_pieces.QATrainPieces.from_dataset(ds).to("cuda"), qa_train_arena.QATrainArena.from_dataset(ds).to("cuda"), meta, tok


def first_epoch(meta):
    first = meta["epochs"][0]
    return [(bi, first[lo:lo + meta["batch"]]) for bi, lo in enumerate(range(0, len(first), meta["batch"]))]


def test_fixture_batches_equal_the_host_composition_and_the_reference(fixture_arenas):
    pieces, _, meta, tok = fixture_arenas
    z = np.load(os.path.join(GOLD, "qa_train_ref.npz"))
    for bi, idx in first_epoch(meta):
        L, S, P = pieces.batch_shape(idx)
        got = guarded_call(pieces, idx, L, S, P, tok.pad_token_id)
        assert_same(got, pieces.compose_host(idx, pad_id=tok.pad_token_id), f"batch {bi}")
        for k in (k.split(".", 1)[1] for k in z.files if k.startswith(f"b{bi}.")):
            assert np.array_equal(got[k], z[f"b{bi}.{k}"]), (bi, k)  # the reference's qa_collate itself
        again = guarded_call(pieces, idx, L, S, P, tok.pad_token_id)
        assert all(got[k].tobytes() == again[k].tobytes() for k in got), "two runs differ"


def test_compose_equals_the_item_arenas_kernel(fixture_arenas):
    pieces, items, meta, tok = fixture_arenas
    n = items.n
    rng = np.random.default_rng(5)
    lists = [idx for _, idx in first_epoch(meta)] + [list(range(n)), [-1, 0, n, 0], list(rng.permutation(n)) + list(rng.permutation(n)[:9])]
    for idx in lists:
        for widths in (items.batch_shape(idx), (20, 2, 2)):
            assert pieces.batch_shape(idx) == items.batch_shape(idx)
            on_dev = torch.tensor(idx, dtype=torch.int64, device="cuda")
            a, b = pieces.assemble(on_dev, *widths, tok.pad_token_id), items.assemble(on_dev, *widths, tok.pad_token_id)
            assert sorted(a) == sorted(b)
            for k in a:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (idx, widths, k)


# ---- random piece arenas ---------------------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def random_arrays():
    """The integer arrays of the random arena (everything but the cuts): 6 questions, 12 passages, 16 items."""
    rng = np.random.default_rng(17)
    cum = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int64)  # noqa: E731
    q_lens = [Q_MAX, 0, 3, 7, 1, Q_MAX]
    p_lens = [9, 600, 7, 0, 40, 1, 23, 0, 12, 5, 31, 16]
    p_ns = [3, 9, 2, 0, 6, 1, 0, 0, 4, 0, 5, 2]  # passages 3 and 7 hold no token; 6 and 9 tokens but no sentence
    starts = [np.sort(rng.choice(n, k, replace=False)) if k else np.zeros(0, np.int64) for n, k in zip(p_lens, p_ns)]
    # (question, P1, P2): the two targets under the longest question, the all-in-P2 item, then the edge passages and random rest
    chains = [(0, 0, 2), (5, 1, 4), (0, 0, 8), (1, 3, 7), (1, 3, 0), (2, 5, 3), (3, 6, 9), (4, 4, 4), (1, 1, 1)] + \
             [(int(rng.integers(0, 6)), int(rng.integers(0, 12)), int(rng.integers(0, 12))) for _ in range(7)]
    n = len(chains)
    label, cov = rng.integers(0, 2, n), rng.integers(0, 2, n)
    ns = [p_ns[a] + p_ns[b] for _, a, b in chains]
    labelled = [i % 3 != 1 for i in range(n)]  # every third item holds no labels
    labelled[SMALL] = labelled[BIG] = True
    n_pairs = [6, 7, 5, 0, 2, 1, 0, 4, 3] + [int(x) for x in rng.integers(0, 5, 7)]  # more than n_span = 3; none
    spans = []
    for i, (_, a, b) in enumerate(chains):
        wp = 4 + p_lens[a] + p_lens[b]
        lo = 4 + p_lens[a] if i == ALL_IN_P2 else 0
        first = rng.integers(lo, wp + 3, n_pairs[i])  # some start behind the chain's end
        if i in (SMALL, BIG):
            first[:3] = (0, 2 + p_lens[a] // 2, 3 + p_lens[a])  # yes; inside P1 and on its separator: they straddle the cuts behind them
        spans.extend((int(f), int(f + w)) for f, w in zip(first, rng.integers(0, 12, n_pairs[i])))
    return dict(q_tokens=rng.integers(1, 500, sum(q_lens)), q_offsets=cum(q_lens), p_tokens=rng.integers(1, 500, sum(p_lens)), p_offsets=cum(p_lens),
                p_sent_starts=np.concatenate(starts).astype(np.int32), p_sent_offsets=cum(p_ns), items=np.array([c + (int(label[i]), int(cov[i])) for i, c in enumerate(chains)]),
                sent_label=rng.integers(0, 2, sum(k for k, on in zip(ns, labelled) if on)), sent_label_index=cum([k if on else 0 for k, on in zip(ns, labelled)]),
                spans=np.array(spans).reshape(-1, 2), span_index=cum(n_pairs), special=SPECIAL)


def max_seq_len_for(target, cut):
    """The max_seq_len at which the target item's chain is cut at `cut`."""
    a = random_arrays()
    q, c0, c1 = (int(x) for x in a["items"][target][:3])
    ql, l0, l1 = (int(np.diff(a[k])[r]) for k, r in (("q_offsets", q), ("p_offsets", c0), ("p_offsets", c1)))
    assert ql == Q_MAX and l0 >= 2 and l1 >= 2
    n_wp = {CUTS[0]: 3, CUTS[1]: 3 + l0 // 2, CUTS[2]: 3 + l0, CUTS[3]: 4 + l0, CUTS[4]: 4 + l0 + l1 // 2, CUTS[5]: 4 + l0 + l1 + 50}[cut]
    return ql + 2 + n_wp + 1


@functools.lru_cache(maxsize=None)
def host_arena(max_seq_len):
    from multihop_dense_retrieval_amd import qa_train_pieces
    return qa_train_pieces.QATrainPieces(**random_arrays(), cuts=[max_seq_len, Q_MAX])


def device_arena(max_seq_len):
    arena = host_arena(max_seq_len)
    return arena if arena.dev is not None else arena.to("cuda")


def indices_for(rows, out_len):
    n = len(random_arrays()["items"])
    rng = np.random.default_rng(rows * 1000 + out_len)
    i, j, k = (int(x) for x in rng.integers(3, n, 3))
    target = BIG if out_len >= 257 else SMALL
    if rows == 1:
        return target, [target]
    if rows == 3:
        return target, [-1, target, n]
    return target, [i, i, -1, target, n, ALL_IN_P2, k if j == i else j]  # a repeated index, both sides outside the arena


@functools.lru_cache(maxsize=None)
def expected(rows, out_len, cut, n_sent, n_span):
    """compose_host of one grid point, computed once and shared by the kernel's test and the test of the grid itself."""
    target, idx = indices_for(rows, out_len)
    msl = max_seq_len_for(target, cut)
    want = host_arena(msl).compose_host(idx, out_len, n_sent, n_span, pad_id=7)
    for v in want.values():
        v.setflags(write=False)
    return msl, idx, want


@pytest.mark.parametrize("out_len", OUT_LENS)
@pytest.mark.parametrize("rows", ROWS)
def test_random_arena_grid(rows, out_len):
    for cut in CUTS:
        for n_sent in N_SENTS:
            for n_span in N_SPANS:
                msl, idx, want = expected(rows, out_len, cut, n_sent, n_span)
                arena = device_arena(msl)
                got = guarded_call(arena, idx, out_len, n_sent, n_span, 7)
                assert_same(got, want, (cut, idx, n_sent, n_span))
                again = guarded_call(arena, idx, out_len, n_sent, n_span, 7)
                assert all(got[k].tobytes() == again[k].tobytes() for k in got), "two runs differ"


def test_the_grid_holds_its_cases():
    """On the expected outputs (no device work): the cases the grid is for occur in it."""
    a = random_arrays()
    p_lens, q_lens = np.diff(a["p_offsets"]), np.diff(a["q_offsets"])
    assert 0 in p_lens and 600 in p_lens and 0 in q_lens and q_lens.max() == Q_MAX and 0 in np.diff(a["p_sent_offsets"])[p_lens > 0]
    assert 0 in np.diff(a["sent_label_index"]) and 0 in np.diff(a["span_index"]) and np.diff(a["span_index"]).max() > max(N_SPANS)
    seen = set()
    for rows in ROWS:
        for out_len in OUT_LENS:
            target, idx = indices_for(rows, out_len)
            t = idx.index(target)
            q, c0, c1 = (int(x) for x in a["items"][target][:3])
            l0, l1, po = int(p_lens[c0]), int(p_lens[c1]), int(q_lens[q]) + 2
            for cut in CUTS:
                msl, _, want = expected(rows, out_len, cut, max(N_SENTS), max(N_SPANS))
                host = host_arena(msl)
                n_wp = int(want["lengths"][t]) - po - 1
                assert n_wp == {CUTS[0]: 3, CUTS[1]: 3 + l0 // 2, CUTS[2]: 3 + l0, CUTS[3]: 4 + l0, CUTS[4]: 4 + l0 + l1 // 2, CUTS[5]: 4 + l0 + l1}[cut]
                ids = want["input_ids"][t]
                if po + n_wp < out_len:
                    assert ids[po + n_wp] == SPECIAL[1] and (ids[po + n_wp + 1:] == 7).all()  # [SEP] closes the row where the cut falls
                if cut == CUTS[3] and po + n_wp <= out_len:
                    assert ids[po + n_wp - 1] == SPECIAL[1]  # the separator behind P1 is the last kept WordPiece
                if cut == CUTS[1] and target == BIG:
                    seen.add("P1 alone passes the cut")
                    assert n_wp < 3 + 600
                if out_len > 256 and int(want["lengths"][t]) > 256:
                    seen.add("a thread walks its stride more than once over real tokens")
                if (want["lengths"] > out_len).any():
                    seen.add("a row longer than out_len")
                for r, i in enumerate(idx):
                    if not 0 <= i < host.n:
                        assert want["label"][r, 0] == -1 and (want["input_ids"][r] == 7).all() and (want["starts"][r] == -1).all() and want["lengths"][r] == 0
                        seen.add("index -1" if i < 0 else "index N")
                        continue
                    pairs = host.spans[host.span_index[i]:host.span_index[i + 1]]
                    cut_r = int(host.n_wp[i])
                    inside = pairs[pairs[:, 0] < cut_r]
                    if len(pairs) and not len(inside):
                        assert want["starts"][r, 0] == -1 and want["ends"][r, 0] == -1
                        seen.add("pairs all behind the cut give (-1, -1)")
                    if len(inside) > max(N_SPANS):
                        seen.add("more pairs than n_span")
                    k = min(len(inside), max(N_SPANS))
                    if (inside[:k, 1] > cut_r - 1).any():
                        assert (want["ends"][r, :k] <= po_of(host, i) + cut_r - 1).all()
                        seen.add("a straddling pair is clamped")
                    if len(inside) < len(pairs) and len(inside) and (pairs[:len(inside), 0] >= cut_r).any():
                        seen.add("kept pairs are compacted over a dropped one")
                    if host.n_sents[i] > max(N_SENTS):
                        seen.add("more sentences than n_sent")
                    if host.n_sents[i] < host.p_n_sents[host.items[i, 1:3]].sum():
                        seen.add("sentences behind the cut")
                    if host.sent_label_index[i + 1] == host.sent_label_index[i] and host.n_sents[i]:
                        assert not want["sent_labels"][r].any()
                        seen.add("an item without labels")
                    if want["sent_labels"][r].any():
                        seen.add("a label of 1")
    assert seen == {"P1 alone passes the cut", "a thread walks its stride more than once over real tokens", "a row longer than out_len", "index -1", "index N",
                    "pairs all behind the cut give (-1, -1)", "more pairs than n_span", "a straddling pair is clamped",
                    "kept pairs are compacted over a dropped one", "more sentences than n_sent", "sentences behind the cut", "an item without labels",
                    "a label of 1"}, seen


def po_of(host, i):
    return int(host.para_offset[i])


def test_bad_arguments_are_refused():
    from multihop_dense_retrieval_amd import _lib
    arena = device_arena(max_seq_len_for(SMALL, CUTS[5]))
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
    # the entry point's own check: max_seq_len leaves no room for yes no [SEP] behind the longest stored question (the class refuses it earlier)
    arena.max_seq_len = Q_MAX + 5
    try:
        with pytest.raises(_lib.MdrError, match="leaves no room"):
            arena.assemble(idx, 8, 1, 1)
    finally:
        arena.max_seq_len = int(arena.cuts[0])
