"""GPU (-m gpu): the reader's evaluation split over several ranks (qa_eval.score_table with a world), the ranks emulated in
one process by dist.LoopbackWorld on the committed tiny ELECTRA, with --sp-pred, and both dev fixtures, each cut into ONE batch (fewer
batches than ranks: all but rank 0 decode nothing) and into FIVE, for N in {2, 3}.

Every emulated rank's merged table equals the one-rank score_table in all five tensors and both lists, bit for bit; from it
predict_metrics returns the same dict and best_res and logs the same lines, and final_results returns the same dict. Every rank decodes
whole batches of its own run only (counted), and the one-rank table of each cut is computed once."""
import json
import os
import types

import pytest
import torch

from test_qa_eval_host import FIXTURES, logged

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny")
CUTS = {("reader", 1): 15, ("reader", 5): 3, ("train", 1): 29, ("train", 5): 6}  # --predict_batch_size for 15 and 29 chains


@pytest.fixture(scope="module")
def tok():
    import transformers
    return transformers.BertTokenizer(os.path.join(ASSETS, "vocab.txt"), do_lower_case=True)


@pytest.fixture(scope="module")
def model():
    import transformers
    from multihop_dense_retrieval_amd import reader
    cfg = transformers.AutoConfig.from_pretrained(ASSETS, local_files_only=True)
    m = reader.QAModel(cfg, types.SimpleNamespace(model_name="electra-tiny", sp_pred=True))
    reader.load_saved(m, os.path.join(ASSETS, "ckpt.pt"), exact=False, map_location="cpu")
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def one_rank(tok, model):
    """{(fixture, batches): (pieces, the one-rank table, its predict_metrics with lines for both sweeps, its final_results)}, computed once."""
    from multihop_dense_retrieval_amd import qa_eval
    out = {}
    for (name, n_batches), bs in CUTS.items():
        path, full, max_q_len, _, _ = FIXTURES[name]
        pieces = qa_eval.QAEvalPieces.from_file(path, tok, full, max_q_len, bs).to(torch.device("cuda", 0))
        assert len(pieces.batches) == n_batches
        table = qa_eval.score_table(model, pieces, 35)
        metrics = {fixed: logged("reader-multirank-eval-one", lambda lg, f=fixed: qa_eval.predict_metrics(pieces, table, tok, True, lg, fixed_thresh=f))
                   for fixed in (None, 0.8)}
        out[name, n_batches] = (pieces, table, metrics, qa_eval.final_results(pieces, table, tok, True))
    return out


class Counting:
    """The model, counting the rows of every decode() call."""

    def __init__(self, model):
        self.model, self.rows = model, []

    def decode(self, net, max_ans_len):
        self.rows.append(int(net["input_ids"].shape[0]))
        return self.model.decode(net, max_ans_len)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("n_batches", [1, 5])
@pytest.mark.parametrize("name", sorted(FIXTURES))
@pytest.mark.parametrize("N", [2, 3])
def test_every_rank_holds_the_one_rank_table_and_evaluates_the_same(tok, model, one_rank, N, name, n_batches):
    from multihop_dense_retrieval_amd import dist, qa_eval
    pieces, want, want_metrics, want_final = one_rank[name, n_batches]
    assert want.sp_prob is not None and want.batch_lo == [lo for lo, _ in pieces.batches]
    deal = qa_eval.batch_deal(n_batches, N)
    models = [Counting(model) for _ in range(N)]
    tables = dist.LoopbackWorld(N).run(lambda w: qa_eval.score_table(models[w.rank], pieces, 35, world=w))
    for r, got in enumerate(tables):
        assert models[r].rows == [hi - lo for lo, hi in pieces.batches[deal[r][0]:deal[r][1]]], (r, "a rank decodes its own whole batches")
        for t in ("rank16", "span16", "start", "end", "sp_prob"):
            assert getattr(got, t).is_cuda and same_bits(getattr(got, t), getattr(want, t)), (r, t)
        assert got.batch_lo == want.batch_lo and got.batch_sents == want.batch_sents, r
        for fixed in (None, 0.8):
            (w_metrics, w_best), w_lines = want_metrics[fixed]
            (metrics, best), lines = logged(f"reader-multirank-eval-{r}", lambda lg, f=fixed: qa_eval.predict_metrics(pieces, got, tok, True, lg, fixed_thresh=f))
            assert lines == w_lines and len(lines) == 3 + 7 * (11 if fixed is None else 1), (r, fixed)
            assert json.dumps(metrics) == json.dumps(w_metrics) and json.dumps(best) == json.dumps(w_best), (r, fixed)
        assert json.dumps(qa_eval.final_results(pieces, got, tok, True)) == json.dumps(want_final), r
    assert sum(len(m.rows) for m in models) == n_batches and (n_batches >= N or models[-1].rows == [])
