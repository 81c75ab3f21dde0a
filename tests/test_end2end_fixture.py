"""CPU (-m "not gpu"): the end-to-end CLI's host pieces against what the REFERENCE'S OWN scripts/end2end.py computed on toy assets
(tests/golden/end2end_ref.{json,npz}, written by scripts/gen_end2end_golden.py; the assets are rebuilt here from seeds).

1. From the reference's captured chains, the QA arena + assemble_host reproduce its collated reader tensors exactly, batch by batch.
2. Fed the reference's captured fp32 head outputs, end2end.select_and_decode reproduces its --save-prediction bytes and end2end.answer_line
   its `Answer EM ..., F1 ...` line exactly."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from oracle import gen_cli_golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
READER = os.path.join(GOLD, "reader_electra_tiny")


@pytest.fixture(scope="module")
def ref():
    return json.load(open(os.path.join(GOLD, "end2end_ref.json"))), np.load(os.path.join(GOLD, "end2end_ref.npz"))


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    from scripts.gen_end2end_golden import corpus_with_sents
    from multihop_dense_retrieval_amd import qa_arena
    a = gen_cli_golden.build_assets(str(tmp_path_factory.mktemp("e2e_fixture")))
    corpus = corpus_with_sents(a["docs"])
    tok = transformers.BertTokenizer(os.path.join(READER, "vocab.txt"), do_lower_case=True)
    items = [json.loads(line) for line in open(a["raw_small"])]
    return {"corpus": corpus, "tok": tok, "items": items, "arena": qa_arena.QAArena.from_corpus(corpus, tok)}


def _batches(case, items):
    """The reference's reader batches: DataLoader(batch_size=topk) over one question's topk chains each."""
    assert case["n_batches"] == len(items) == len(case["chains"])
    return [(items[b], case["chains"][b]) for b in range(len(items))]


@pytest.mark.parametrize("name", ["k1_b1", "k3_b2_sp", "k4"])
def test_host_pieces_reproduce_the_reference_collated_tensors(ref, toy, name):
    from multihop_dense_retrieval_amd import end2end, qa_arena
    meta, z = ref
    case = meta["cases"][name]
    special = qa_arena.special_ids(toy["tok"])
    for bi, (item, chains) in enumerate(_batches(case, toy["items"])):
        q_ids = end2end.question_ids(toy["tok"], [item["question"]])
        got = qa_arena.assemble_host(toy["arena"], q_ids, chains, [0] * len(chains), special, end2end.READER_MAX_SEQ_LEN)
        for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets"):
            want = z[f"{name}.b{bi}.{k}"]
            assert got[k].shape == want.shape and np.array_equal(got[k], want.astype(np.int64)), (bi, k)
        assert got["para_offsets"].tolist() == case["para_offsets"][bi]


def reference_heads(z, name, bi, sp_pred, max_ans_len=35):
    """eval_final's device-side work on the reference's own fp32 outputs (its formula, in the outputs' dtype)."""
    from multihop_dense_retrieval_amd import reader
    s, e = torch.from_numpy(z[f"{name}.b{bi}.start_logits"]), torch.from_numpy(z[f"{name}.b{bi}.end_logits"])
    st, en, sc = reader.span_search_reference(s, e, max_ans_len)
    out = {"start": st.tolist(), "end": en.tolist(), "span_score": sc.tolist(), "rank_score": z[f"{name}.b{bi}.rank_score"].reshape(-1).tolist(),
           "sp_prob": None}
    if sp_pred:
        so = torch.from_numpy(z[f"{name}.b{bi}.sent_offsets"])
        out["sp_prob"] = torch.from_numpy(z[f"{name}.b{bi}.sp_score"]).masked_fill(so.eq(0), float("-inf")).sigmoid().tolist()
    return out


@pytest.mark.parametrize("name", ["k1_b1", "k3_b2_sp", "k4"])
def test_selection_and_decode_reproduce_the_reference_prediction_and_answer_line(ref, toy, name, tmp_path):
    from multihop_dense_retrieval_amd import end2end
    meta, z = ref
    case = meta["cases"][name]
    sp_pred = "--sp-pred" in case["flags"]
    results = {"answer": {}, "sp": {}, "titles": {}}
    for bi, (item, chains) in enumerate(_batches(case, toy["items"])):
        q_ids = end2end.question_ids(toy["tok"], [item["question"]])
        psg = [[[toy["corpus"][str(a)], toy["corpus"][str(c)]] for a, c in chains]]
        for qid, ans in end2end.select_and_decode([item], reference_heads(z, name, bi, sp_pred), psg, [len(q_ids[0]) + 2], toy["tok"], sp_pred):
            results["answer"][qid], results["sp"][qid], results["titles"][qid] = ans["pred_str"], ans["pred_sp"], ans["chain_titles"]
    p = tmp_path / "pred.json"
    with open(p, "w") as f:
        json.dump(results, f)
    assert p.read_text() == case["save_prediction"]
    gold = {it["_id"]: it["answer"][0] for it in toy["items"]}
    assert end2end.answer_line(results, gold) == case["log"][-1]
    assert case["stdout"] == [f"Total instances size {len(toy['items']) * len(case['chains'][0])}", "Finishing evaluation in <s>"]
    if sp_pred:
        assert any(v for v in results["sp"].values())  # the sp branch is exercised
