"""CPU (-m "not gpu"): the QA passage arena (multihop_dense_retrieval_amd/qa_arena.py). qa_arena.assemble_host -- the yardstick of the
mdr_reader_assemble kernel -- must equal QAEvalDataset + qa_collate exactly (every tensor, para_offsets and the wp tokens) on the reader
fixture's chains and on edge cases of prepare()'s whitespace rule; the cache tag must force a rebuild when the vocabulary changes."""
import copy
import os

import numpy as np
import pytest

transformers = pytest.importorskip("transformers")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny")
MAX_SEQ, MAX_Q = 512, 64


@pytest.fixture(scope="module")
def tok():
    return transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)


def _long(n, k, word="the"):
    return " ".join([word] * n) + (" ." if k % 2 else "")


def edge_corpus():
    """Passages that exercise prepare()'s rule: literal specials inside sentences, an empty title, no sentences, Zs spaces (both rules split
    on them) and \\x0b / \\x85 / \\u2028 inside a word (only str.split() would split there), accents and ## pieces, long passages."""
    return [
        {"title": "Rock Film", "sents": ["the film was released first .", "john paul was born in paris ."]},
        {"title": "", "sents": ["an empty title .", "second sentence ."]},
        {"title": "No Sentences", "sents": []},
        {"title": "Literal", "sents": ["a literal [unused1] marker inside .", "and a [SEP] inside , [unused2] too ."]},
        {"title": "Spaces Zs", "sents": ["non breaking　spaces here .", "tab\tand\nnewline ."]},
        {"title": "Odd", "sents": ["word\x0bjoined and\x85more and line ."]},
        {"title": "Café Zürich", "sents": ["bjork played singing loudly .", "  padded sentence  "]},
        {"title": "Long one", "sents": [_long(60, i) for i in range(6)]},
        {"title": "Long two", "sents": [_long(50, i, "york") for i in range(5)]},
        {"title": "  ", "sents": [""]},
    ]


def _collate_rows(tok, questions, corpus, chains, row_q):
    from multihop_dense_retrieval_amd import qa_data
    items = [{"_id": f"q{r}", "question": questions[row_q[r]], "candidate_chains": [[copy.deepcopy(corpus[c]) for c in chains[r]]]}
             for r in range(len(chains))]
    ds = qa_data.QAEvalDataset(tok, items, max_seq_len=MAX_SEQ, max_q_len=MAX_Q)
    return qa_data.qa_collate([ds[i] for i in range(len(ds))], pad_id=tok.pad_token_id)


def _check_equal(tok, arena, questions, corpus, chains, row_q):
    from multihop_dense_retrieval_amd import qa_arena
    ref = _collate_rows(tok, questions, corpus, chains, row_q)
    q_ids = [qa_arena.question_ids(tok, q, MAX_Q) for q in questions]
    got = qa_arena.assemble_host(arena, q_ids, chains, row_q, qa_arena.special_ids(tok), MAX_SEQ)
    for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets"):
        want = ref["net_inputs"][k]
        assert got[k].shape == tuple(want.shape), (k, got[k].shape, tuple(want.shape))
        assert np.array_equal(got[k], want.numpy().astype(np.int64)), k
    assert got["para_offsets"].tolist() == ref["para_offsets"]
    assert [w.tolist() for w in got["wp_ids"]] == [tok.convert_tokens_to_ids(w) for w in ref["wp_tokens"]]
    assert got["lengths"].tolist() == ref["net_inputs"]["attention_mask"].sum(1).tolist()
    return ref


def test_assemble_host_equals_collate_on_the_reader_fixture(tok):
    import json
    from multihop_dense_retrieval_amd import qa_arena
    items = [json.loads(line) for line in open(os.path.join(ASSETS, "items.jsonl"))]
    corpus, key, chains, row_q, questions = [], {}, [], [], []
    for qi, it in enumerate(items):
        questions.append(it["question"])
        for ch in it["candidate_chains"]:
            ids = []
            for p in ch:
                k = json.dumps(p, sort_keys=True)
                if k not in key:
                    key[k] = len(corpus)
                    corpus.append(p)
                ids.append(key[k])
            chains.append(ids)
            row_q.append(qi)
    arena = qa_arena.QAArena.from_corpus({str(i): d for i, d in enumerate(corpus)}, tok)
    ref = _check_equal(tok, arena, questions, corpus, chains, row_q)
    # the fixture holds a chain cut at max_seq_len and a question longer than max_q_len
    assert max(ref["para_offsets"]) == MAX_Q + 2
    assert any(len(w) == MAX_SEQ - po - 1 for w, po in zip(ref["wp_tokens"], ref["para_offsets"]))


def test_assemble_host_equals_collate_on_edge_cases(tok):
    from multihop_dense_retrieval_amd import qa_arena
    corpus = edge_corpus()
    arena = qa_arena.QAArena.from_corpus({str(i): d for i, d in enumerate(corpus)}, tok)
    questions = ["which film was released first?", "is it  yes ?", " ".join(["paris"] * 90) + "?", "café zürich??"]
    n = len(corpus)
    chains = [[a, b] for a in range(n) for b in range(n)]
    row_q = [i % len(questions) for i in range(len(chains))]
    ref = _check_equal(tok, arena, questions, corpus, chains, row_q)
    # edge cases are really exercised: a row cut mid-passage with sentence starts past the cut, a literal [unused1] counted as a start
    cut = [i for i, (w, po) in enumerate(zip(ref["wp_tokens"], ref["para_offsets"])) if len(w) == MAX_SEQ - po - 1]
    assert cut and any(len(ref["net_inputs"]["sent_offsets"][i].nonzero()) < arena.n_sents[chains[i]].sum() for i in cut)
    assert arena.n_sents[3] == 3 and arena.n_sents[2] == 0
    # \x0b, \x85 and   stay inside words (str.split() would split there)
    assert qa_arena.split_words("a\x0bb c\x85d e f g h") == ["a\x0bb", "c\x85d", "e f", "g", "h"]


def test_row_geometry_and_out_of_range_ids(tok):
    from multihop_dense_retrieval_amd import qa_arena
    corpus = edge_corpus()
    arena = qa_arena.QAArena.from_corpus({str(i): d for i, d in enumerate(corpus)}, tok)
    q_ids = [qa_arena.question_ids(tok, "which film", MAX_Q)]
    sp = qa_arena.special_ids(tok)
    out = qa_arena.assemble_host(arena, q_ids, [[-1, len(corpus)], [0, 10 ** 9]], [0, 0], sp, MAX_SEQ)
    empty = [sp["cls"]] + q_ids[0] + [sp["sep"], sp["yes"], sp["no"], sp["sep"], sp["sep"], sp["sep"]]
    assert out["input_ids"][0, :len(empty)].tolist() == empty and out["lengths"][0] == len(empty)
    L, S = arena.batch_shape([len(q_ids[0])], [[7, 8], [0, 1]], [0, 0], MAX_SEQ)
    assert L == MAX_SEQ and S > 0


def test_memoised_build_equals_plain_and_parallel_build(tok):
    from multihop_dense_retrieval_amd import qa_arena
    corpus = {str(i): d for i, d in enumerate(edge_corpus() * 3)}
    a = qa_arena.QAArena.from_corpus(corpus, tok, memo=True, chunk=4)
    b = qa_arena.QAArena.from_corpus(corpus, tok, memo=False, chunk=4)
    c = qa_arena.QAArena.from_corpus(corpus, tok, workers=3, chunk=4)
    for x in (b, c):
        for k in ("tokens", "offsets", "sent_starts", "sent_offsets"):
            assert np.array_equal(getattr(a, k), getattr(x, k)), k


def test_cache_tag_forces_rebuild_when_the_vocabulary_changes(tok, tmp_path):
    from multihop_dense_retrieval_amd import qa_arena
    corpus = {str(i): d for i, d in enumerate(edge_corpus())}
    path = str(tmp_path / "corpus.json")
    a = qa_arena.QAArena.load_or_build(path, corpus, tok)
    assert os.path.exists(path + ".qa_arena.npz")
    b = qa_arena.QAArena.load(path + ".qa_arena.npz", expect_tag=qa_arena.qa_arena_tag(tok))
    assert b is not None and np.array_equal(np.asarray(b.tokens), a.tokens)
    vocab = open(os.path.join(ASSETS, "vocab.txt")).read().split("\n")
    (tmp_path / "v2.txt").write_text("\n".join([v for v in vocab if v != "film"]))
    tok2 = transformers.BertTokenizer(str(tmp_path / "v2.txt"), do_lower_case=True)
    assert qa_arena.qa_arena_tag(tok2) != qa_arena.qa_arena_tag(tok)
    assert qa_arena.QAArena.load(path + ".qa_arena.npz", expect_tag=qa_arena.qa_arena_tag(tok2)) is None
    c = qa_arena.QAArena.load_or_build(path, corpus, tok2)
    assert not np.array_equal(c.tokens, a.tokens)
    assert qa_arena.QAArena.load(path + ".qa_arena.npz", expect_tag=qa_arena.qa_arena_tag(tok2)) is not None
    # a cache for another passage count (an edited corpus under the same name) is rebuilt too
    bigger = dict(corpus, **{str(len(corpus)): {"title": "New", "sents": ["one more passage ."]}})
    d = qa_arena.QAArena.load_or_build(path, bigger, tok2)
    assert d.n == len(bigger) and qa_arena.QAArena.load(path + ".qa_arena.npz").n == len(bigger)
    # lower-casing is part of the tag too
    tok3 = transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=False)
    assert qa_arena.qa_arena_tag(tok3) != qa_arena.qa_arena_tag(tok)


def test_special_ids_refuse_a_multi_piece_yes(tmp_path):
    from multihop_dense_retrieval_amd import qa_arena
    vocab = open(os.path.join(ASSETS, "vocab.txt")).read().split("\n")
    (tmp_path / "v.txt").write_text("\n".join([v for v in vocab if v != "yes"]))
    with pytest.raises(ValueError):
        qa_arena.special_ids(transformers.BertTokenizer(str(tmp_path / "v.txt"), do_lower_case=True))
