"""GPU (-m gpu): the reader's evaluation from the dev piece arena (multihop_dense_retrieval_amd/qa_eval.py) against the host path, on the
committed tiny ELECTRA and both fixtures: the rows mdr_reader_assemble writes for every batch equal qa_collate's bit for bit; the score
table after the arena sweep holds the bits decode() returns for the host path's batches; and scripts/train_qa.py's evaluation through
either path (run_batches + qa_data.predict_metrics / final_results, or qa_eval.score_table + qa_eval.predict_metrics / final_results,
with mdr_reader_select choosing the chains) logs the same lines and returns the same objects, with and without --sp-pred."""
import json
import os
import types

import numpy as np
import pytest
import torch

from test_qa_eval_host import FIXTURES, assert_rows_equal, host_batches, load_script, logged

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny")
BATCH = {"reader": 4, "train": 8}


@pytest.fixture(scope="module")
def tok():
    import transformers
    return transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)


@pytest.fixture(scope="module")
def models():
    import transformers
    from multihop_dense_retrieval_amd import reader
    cfg = transformers.AutoConfig.from_pretrained(ASSETS, local_files_only=True)
    out = {}
    for sp_pred in (True, False):
        m = reader.QAModel(cfg, types.SimpleNamespace(model_name="electra-tiny", sp_pred=sp_pred))
        reader.load_saved(m, os.path.join(ASSETS, "ckpt.pt"), exact=False, map_location="cpu")
        out[sp_pred] = m.to("cuda").eval()
    return out


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_device_rows_equal_qa_collate(tok, name):
    from multihop_dense_retrieval_amd import qa_eval
    path, full, max_q_len, cuts, _ = FIXTURES[name]
    for max_seq_len, bs in ((full, BATCH[name]), (full, 64), (cuts[0], 4), (cuts[1], 1)):
        pieces = qa_eval.QAEvalPieces.from_file(path, tok, max_seq_len, max_q_len, bs).to(torch.device("cuda", 0))
        batches = host_batches(tok, path, max_seq_len, max_q_len, bs)
        assert len(batches) == len(pieces.batches)
        for (lo, hi), b in zip(pieces.batches, batches):
            rows = pieces.assemble(lo, hi)
            assert all(t.is_cuda and t.dtype == torch.int64 for t in rows.values())
            got = {k: v.cpu().numpy() for k, v in rows.items()}
            assert_rows_equal(got, b, (max_seq_len, bs, lo))
            want = pieces.assemble_host(lo, hi)
            assert all(np.array_equal(got[k], want[k]) for k in got), (max_seq_len, bs, lo)


@pytest.mark.parametrize("name", sorted(FIXTURES))
@pytest.mark.parametrize("sp_pred", [True, False], ids=["sp", "nosp"])
def test_score_table_and_evaluation_equal_the_host_path(tok, models, name, sp_pred):
    from multihop_dense_retrieval_amd import qa_data, qa_eval
    script = load_script("train_qa")
    path, full, max_q_len, _, _ = FIXTURES[name]
    bs, model = BATCH[name], models[sp_pred]
    args = types.SimpleNamespace(max_ans_len=35, sp_pred=sp_pred)
    pieces = qa_eval.QAEvalPieces.from_file(path, tok, full, max_q_len, bs).to(torch.device("cuda", 0))
    batches = host_batches(tok, path, full, max_q_len, bs)
    table = qa_eval.score_table(model, pieces, args.max_ans_len)
    assert table.rank16.is_cuda and (table.sp_prob is not None) == sp_pred
    for (lo, hi), b in zip(pieces.batches, batches):  # the host path's decode() of its own batch: the same bits
        head = model.decode(b["net_inputs"], args.max_ans_len)
        same = lambda a, w: torch.equal(a.cpu(), w.cpu())  # noqa: E731
        assert same(table.rank16[lo:hi], head["rank_score"].view(-1).view(torch.int16)) and same(table.span16[lo:hi], head["span_score"].view(torch.int16))
        assert same(table.start[lo:hi], head["start"]) and same(table.end[lo:hi], head["end"])
        if sp_pred:
            S = head["sp_prob"].shape[1]
            assert S == b["net_inputs"]["sent_offsets"].shape[1] == table.sents_of(lo) == table.sents_of(hi - 1)
            assert same(table.sp_prob[lo:hi, :S].view(torch.int16), head["sp_prob"].view(torch.int16))
    for fixed in (None, 0.8):
        chains, gold = script.run_batches(model, batches, args, final=False)
        (want, want_best), want_lines = logged("qa-eval-gpu-host", lambda lg: qa_data.predict_metrics(chains, gold, sp_pred, lg, fixed_thresh=fixed))
        (got, got_best), got_lines = logged("qa-eval-gpu-arena", lambda lg: qa_eval.predict_metrics(pieces, table, tok, sp_pred, lg, fixed_thresh=fixed))
        assert got_lines == want_lines and len(got_lines) == 3 + 7 * (11 if fixed is None else 1)
        assert json.dumps(got) == json.dumps(want) and json.dumps(got_best) == json.dumps(want_best)
    chains, _ = script.run_batches(model, batches, args, final=True)
    assert json.dumps(qa_eval.final_results(pieces, table, tok, sp_pred)) == json.dumps(qa_data.final_results(chains, weight=0.8))
    w = qa_eval.Winners(pieces, table, qa_data.combination_factors(None), tok, sp_pred, final=False)
    hw, hr, hf = qa_eval.select_host(table.rank16.cpu().numpy(), table.span16.cpu().numpy(), pieces.seg_offsets, qa_data.combination_factors(None))
    assert np.array_equal(w.winners, hw) and np.array_equal(w.rank_top, hr) and w.flagged == int(hf.sum()) == 0
    assert 0 < w.distinct <= min(pieces.n, 11 * len(pieces.qids))
