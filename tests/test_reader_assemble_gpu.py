"""GPU (-m gpu): mdr_reader_assemble (include/mdr_reader.h) is BIT-IDENTICAL to qa_arena.assemble_host, itself equal to QAEvalDataset +
qa_collate (tests/test_qa_arena.py): random arenas of 10^4 passages and up to 512 rows, prepare()'s edge cases, a sentence width wider
than needed, a row width narrower than the longest row, and out-of-range passage / question ids."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = {"cls": 5, "sep": 6, "yes": 8, "no": 9, "pad": 0}


def _random_arena(rng, n):
    from multihop_dense_retrieval_amd.qa_arena import QAArena
    lens = rng.integers(0, 260, n)
    lens[:3] = [0, 1, 600]
    ns = np.minimum(rng.integers(0, 6, n), lens)
    starts, offs = [], np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    for L, k in zip(lens, ns):
        starts.extend(np.sort(rng.choice(L, k, replace=False)).tolist() if k else [])
    soffs = np.zeros(n + 1, np.int64)
    soffs[1:] = np.cumsum(ns)
    return QAArena(rng.integers(10, 30000, int(offs[-1])).astype(np.int32), offs, np.asarray(starts, np.int32), soffs)


def _run(arena, q_ids, chains, row_q, max_seq_len=512, out_len=None, n_sent=None):
    from multihop_dense_retrieval_amd import qa_arena
    want = qa_arena.assemble_host(arena, q_ids, chains, row_q, SPECIAL, max_seq_len, out_len, n_sent)
    L, S = want["input_ids"].shape[1], want["sent_offsets"].shape[1]
    Lq = max(1, max(len(q) for q in q_ids))
    qt = np.zeros((len(q_ids), Lq), np.int64)
    for b, q in enumerate(q_ids):
        qt[b, :len(q)] = q
    dev = torch.device("cuda", 0)
    got = qa_arena.assemble(arena, torch.from_numpy(qt).to(dev), torch.tensor([len(q) for q in q_ids], device=dev),
                            torch.as_tensor(np.asarray(chains, np.int64), device=dev), torch.as_tensor(np.asarray(row_q, np.int64), device=dev),
                            SPECIAL, max_seq_len, L, S)
    for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets", "para_offsets", "lengths"):
        g = got[k].cpu().numpy()
        assert g.shape == want[k].shape and np.array_equal(g, want[k]), k
    return want


@pytest.mark.parametrize("rows,seed", [(1, 0), (37, 1), (512, 2)])
def test_kernel_is_bit_identical_to_assemble_host_on_random_arenas(rows, seed):
    rng = np.random.default_rng(seed)
    arena = _random_arena(rng, 10_000).to("cuda")
    B = max(1, rows // 5)
    q_ids = [rng.integers(10, 30000, rng.integers(0, 65)).tolist() for _ in range(B)]
    q_ids[0] = rng.integers(10, 30000, 64).tolist()
    chains = rng.integers(0, 10_000, (rows, 2))
    chains[0] = [2, 2]  # 1 200 WordPieces: cut mid-passage, sentence starts past the cut
    row_q = rng.integers(0, B, rows)
    want = _run(arena, q_ids, chains, row_q)
    assert (want["lengths"] == 512).any()
    _run(arena, q_ids, chains, row_q, n_sent=want["sent_offsets"].shape[1] + 7)  # S wider than needed: zero columns
    _run(arena, q_ids, chains, row_q, out_len=300)  # rows longer than out_len are cut, lengths stay unclipped
    _run(arena, q_ids, chains, row_q, max_seq_len=200)


def test_kernel_handles_out_of_range_ids():
    rng = np.random.default_rng(7)
    arena = _random_arena(rng, 1000).to("cuda")
    q_ids = [[11, 12, 13], []]
    chains = [[-1, 5], [1000, 10 ** 12], [3, -7], [0, 1]]
    row_q = [0, 1, 5, -1]  # question indices outside [0, 2): an empty question
    _run(arena, q_ids, chains, row_q)


def test_kernel_on_the_edge_case_corpus_equals_collate():
    transformers = pytest.importorskip("transformers")
    from multihop_dense_retrieval_amd import qa_arena
    from tests.test_qa_arena import ASSETS, _collate_rows, edge_corpus
    tok = transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)
    corpus = edge_corpus()
    arena = qa_arena.QAArena.from_corpus({str(i): d for i, d in enumerate(corpus)}, tok).to("cuda")
    questions = ["which film was released first?", " ".join(["paris"] * 90) + "?"]
    chains = [[a, b] for a in range(len(corpus)) for b in range(len(corpus))]
    row_q = [i % 2 for i in range(len(chains))]
    q_ids = [qa_arena.question_ids(tok, q, 64) for q in questions]
    sp = qa_arena.special_ids(tok)
    L, S = arena.batch_shape([len(q) for q in q_ids], chains, row_q, 512)
    dev = torch.device("cuda", 0)
    qt = torch.zeros((2, 64), dtype=torch.int64)
    for b, q in enumerate(q_ids):
        qt[b, :len(q)] = torch.tensor(q)
    got = qa_arena.assemble(arena, qt.to(dev), torch.tensor([len(q) for q in q_ids], device=dev), torch.tensor(chains, device=dev),
                            torch.tensor(row_q, device=dev), sp, 512, L, S)
    ref = _collate_rows(tok, questions, corpus, chains, row_q)
    for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets"):
        assert torch.equal(got[k].cpu(), ref["net_inputs"][k].to(torch.int64)), k
    assert got["para_offsets"].cpu().tolist() == ref["para_offsets"]
