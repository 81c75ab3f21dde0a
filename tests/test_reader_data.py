"""CPU (-m "not gpu"): the reader's data path (multihop_dense_retrieval_amd/qa_data.py) against fixtures written by EXECUTING the
reference's qa_dataset.py / qa_model.py / train_qa.predict + eval_final (scripts/gen_reader_golden.py): identical collated tensors and
token maps, and -- fed the reference model's own captured head outputs -- identical log lines and --save-prediction bytes."""
import json
import logging
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny")


@pytest.fixture(scope="module")
def ref():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reader_ref.json")))


@pytest.fixture(scope="module")
def npz():
    return np.load(os.path.join(ROOT, "tests", "golden", "reader_batches.npz"))


@pytest.fixture(scope="module")
def batches(ref):
    transformers = pytest.importorskip("transformers")
    from functools import partial
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import qa_data
    tok = transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)
    ds = qa_data.QADataset(tok, os.path.join(ASSETS, "items.jsonl"), ref["max_seq_len"], ref["max_q_len"])
    return list(DataLoader(ds, batch_size=ref["batch_size"], collate_fn=partial(qa_data.qa_collate, pad_id=tok.pad_token_id)))


def test_collate_matches_the_reference(ref, npz, batches):
    assert len(batches) == 4
    chains = [c for b in batches for c in zip(b["qids"], b["para_offsets"], b["wp_tokens"], b["tok_to_orig_index"], b["doc_tokens"])]
    assert [list(c) for c in chains] == [[c["qid"], c["para_offset"], c["wp_tokens"], c["tok_to_orig_index"], c["doc_tokens"]] for c in ref["chains"]]
    for bi, b in enumerate(batches):
        for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets", "label"):
            want = npz[f"b{bi}.{k}"]
            assert np.array_equal(b["net_inputs"][k].numpy(), want) and b["net_inputs"][k].dtype == torch.from_numpy(want).dtype, (bi, k)
    # the fixture exercises what it claims: a truncated chain whose markers fall past max_seq_len, a question cut to max_q_len
    assert any(len(c["wp_tokens"]) == ref["max_seq_len"] - c["para_offset"] - 1 for c in ref["chains"])
    assert max(c["para_offset"] for c in ref["chains"]) == ref["max_q_len"] + 2


def _heads_from_reference(npz, tag, bi, sp_pred, max_ans_len=35):
    from multihop_dense_retrieval_amd import reader
    s, e = torch.from_numpy(npz[f"{tag}.b{bi}.start_logits"]), torch.from_numpy(npz[f"{tag}.b{bi}.end_logits"])
    st, en, sc = reader.span_search_reference(s, e, max_ans_len)
    out = {"start": st.tolist(), "end": en.tolist(), "span_score": sc.tolist(), "rank_score": npz[f"{tag}.b{bi}.rank_score"].reshape(-1).tolist(), "sp_prob": None}
    if sp_pred:
        so = torch.from_numpy(npz[f"b{bi}.sent_offsets"])
        out["sp_prob"] = torch.from_numpy(npz[f"{tag}.b{bi}.sp_score"]).masked_fill(so.eq(0), float("-inf")).sigmoid().tolist()
    return out


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.mark.parametrize("tag", ["sp", "nosp"])
def test_predict_log_lines_and_saved_prediction_match_the_reference(ref, npz, batches, tag, tmp_path):
    from multihop_dense_retrieval_amd import qa_data
    sp_pred = tag == "sp"
    chains, gold = [], {}
    for bi, b in enumerate(batches):
        chains.extend(qa_data.chain_results(b, _heads_from_reference(npz, tag, bi, sp_pred), sp_pred))
        for i, qid in enumerate(b["qids"]):
            gold[qid] = (b["gold_answer"][i], b["sp_gold"][i])
    logger = logging.getLogger("reader-predict-test")
    logger.setLevel(logging.INFO)
    h = _Lines()
    logger.addHandler(h)
    try:
        _, best_res = qa_data.predict_metrics(chains, gold, sp_pred, logger, fixed_thresh=0.8)
    finally:
        logger.removeHandler(h)
    run = ref["runs"][tag]["predict"]
    assert h.lines == run["log"]
    p = tmp_path / "pred.json"
    with open(p, "w") as f:
        json.dump(best_res, f)
    assert p.read_text() == run["save_prediction"]
    if not sp_pred:
        assert run["save_prediction"] == "null"


@pytest.mark.parametrize("tag", ["sp", "nosp"])
def test_eval_final_saved_prediction_matches_the_reference(ref, npz, batches, tag):
    from multihop_dense_retrieval_amd import qa_data
    sp_pred = tag == "sp"
    chains = []
    for bi, b in enumerate(batches):
        chains.extend(qa_data.chain_results(b, _heads_from_reference(npz, tag, bi, sp_pred), sp_pred, final=True))
    assert json.dumps(qa_data.final_results(chains, weight=0.8)) == ref["runs"][tag]["eval_final"]["save_prediction"]


def test_get_final_text_and_metrics():
    from multihop_dense_retrieval_amd import qa_data
    assert qa_data.get_final_text("cafe zurich", "the Café Zürich", do_lower_case=True) == "Café Zürich"
    assert qa_data.get_final_text("xyz", "abc", do_lower_case=True) == "abc"
    assert qa_data.exact_match_score("The  Band!", "band")
    assert qa_data.f1_score("yes", "no") == (0, 0, 0)
    m = {"sp_em": 0, "sp_f1": 0, "sp_prec": 0, "sp_recall": 0}
    assert qa_data.update_sp(m, [["a", 1], ["b", 0]], [["a", 1]]) == (0.0, 0.5, 1.0)


def test_add_sp_labels(tmp_path):
    from multihop_dense_retrieval_amd import qa_data
    raw = [{"question": "q1", "answer": "x", "supporting_facts": [["T1", 0], ["T2", 1], ["T1", 2]]}, {"question": "q2", "answer": "y"}]
    (tmp_path / "raw.json").write_text(json.dumps(raw))
    (tmp_path / "ret.jsonl").write_text("".join(json.dumps({"question": r["question"], "_id": str(i)}) + "\n" for i, r in enumerate(raw)))
    (tmp_path / "t2s.txt").write_text(json.dumps({"title": "T1", "sents": ["a", "b", "c"]}) + "\n" + json.dumps({"title": "T2", "sents": ["d", "e"]}) + "\n")
    qa_data.add_sp_labels(str(tmp_path / "raw.json"), str(tmp_path / "ret.jsonl"), str(tmp_path / "out.jsonl"), str(tmp_path / "t2s.txt"))
    out = [json.loads(line) for line in open(tmp_path / "out.jsonl")]
    assert out[0]["sp"] == [{"title": "T1", "sents": ["a", "b", "c"], "sp_sent_ids": [0, 2]}, {"title": "T2", "sents": ["d", "e"], "sp_sent_ids": [1]}]
    assert out[0]["answer"] == ["x"] and "sp" not in out[1] and "answer" not in out[1]


def test_cli_refuses_training():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_qa.py"), "--do_train"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "training is not supported" in r.stderr
