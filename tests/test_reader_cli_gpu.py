"""GPU (-m gpu): the reader on the fixture assets written by executing the reference (scripts/gen_reader_golden.py).

1. The HIP forward on the fixture checkpoint against the reference QAModel's captured fp32 head outputs (same batches, same weights).
2. scripts/train_qa.py --do_predict (with and without --sp-pred) and --do_test reproduce the reference's log-line formats and predictions.
   The reference ran in fp32, the HIP reader in apex O1 arithmetic; a question's prediction must be equal unless its decision sits inside
   the measured logit error: MARGIN below is the smallest gap (in logit units) between the chosen span and the runner-up span of a chain,
   or between the top two chains' combined scores, below which an item is exempt. The test prints which items were exempt."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ASSETS = os.path.join(GOLD, "reader_electra_tiny")
MARGIN = 0.02  # a span or chain score is a sum of two logits, each within 3.9e-3 of the reference here (measured, test 1), plus one fp16
#                rounding of the sum (<= 4e-3 at these magnitudes): 0.02 leaves about 1.7 x that bound


@pytest.fixture(scope="module")
def ref():
    return json.load(open(os.path.join(GOLD, "reader_ref.json")))


@pytest.fixture(scope="module")
def npz():
    return np.load(os.path.join(GOLD, "reader_batches.npz"))


def _model(sp_pred):
    import types
    from multihop_dense_retrieval_amd import reader
    cfg = transformers.AutoConfig.from_pretrained(ASSETS, local_files_only=True)
    m = reader.QAModel(cfg, types.SimpleNamespace(model_name="electra-tiny", sp_pred=sp_pred))
    reader.load_saved(m, os.path.join(ASSETS, "ckpt.pt"), exact=False, map_location="cpu")
    return m.to("cuda").eval()


@pytest.mark.parametrize("tag", ["sp", "nosp"])
def test_forward_on_fixture_checkpoint_matches_captured_reference_outputs(npz, tag):
    m = _model(tag == "sp")
    worst = 0.0
    for bi in range(4):
        batch = {k: torch.from_numpy(npz[f"b{bi}.{k}"]) for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets")}
        out = m(batch)
        for k in ("start_logits", "end_logits", "rank_score") + (("sp_score",) if tag == "sp" else ()):
            want = torch.from_numpy(npz[f"{tag}.b{bi}.{k}"]).double()
            got = out[k].double().cpu()
            assert torch.equal(torch.isinf(got), torch.isinf(want)), (bi, k)
            fin = torch.isfinite(want)
            worst = max(worst, (got - want)[fin].abs().max().item())
    print(f"[reader fixture {tag}] max |logit err| = {worst:.3e}")
    assert worst < 0.008  # measured 3.9e-3 (MI355X)


def _margins(ref, npz, tag, max_ans_len=35):
    """Per question: smallest runner-up gap of its chains' span decisions and of its chain ranking (0.8 rank + 0.2 span)."""
    from multihop_dense_retrieval_amd import reader
    gaps, scores, ci = {}, {}, 0
    for bi in range(4):
        s, e = torch.from_numpy(npz[f"{tag}.b{bi}.start_logits"]), torch.from_numpy(npz[f"{tag}.b{bi}.end_logits"])
        span = s[:, :, None] + e[:, None]
        L = span.size(1)
        band = torch.ones((L, L), dtype=torch.bool).triu(0).tril(max_ans_len)
        flat = span.masked_fill(~band, -float("inf")).flatten(1)
        top2 = flat.topk(2, dim=1).values
        rank = npz[f"{tag}.b{bi}.rank_score"].reshape(-1)
        for i in range(span.size(0)):
            qid = ref["chains"][ci]["qid"]
            ci += 1
            gaps[qid] = min(gaps.get(qid, np.inf), float(top2[i, 0] - top2[i, 1]))
            scores.setdefault(qid, []).append(0.8 * float(rank[i]) + 0.2 * float(top2[i, 0]))
    for qid, sc in scores.items():
        sc = sorted(sc, reverse=True)
        if len(sc) > 1:
            gaps[qid] = min(gaps[qid], sc[0] - sc[1])
    return gaps


_LOG_FORMATS = [r"evaluated \d+ questions\.\.\.", r"chain ranking em: .+", r"\.\.\.\.\.\.\.Using combination factor 0\.8\.\.\.\.\.\.",
                r"answer em: .+, count: \d+", r"answer f1: .+, count: \d+", r"sp em: .+, count: \d+", r"sp f1: .+, count: \d+",
                r"joint em: .+, count: \d+", r"joint f1: .+, count: \d+", r"Best joint F1 from combination .+"]


@pytest.mark.parametrize("mode,tag", [("predict", "sp"), ("predict", "nosp"), ("eval_final", "sp")])
def test_cli_reproduces_the_reference(ref, npz, tmp_path, mode, tag):
    out = tmp_path / "out.json"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_qa.py"), "--do_predict" if mode == "predict" else "--do_test",
           "--predict_file", os.path.join(ASSETS, "items.jsonl"), "--init_checkpoint", os.path.join(ASSETS, "ckpt.pt"), "--model_name", ASSETS,
           "--fp16", "--max_ans_len", "35", "--max_seq_len", str(ref["max_seq_len"]), "--max_q_len", str(ref["max_q_len"]),
           "--predict_batch_size", str(ref["batch_size"]), "--save-prediction", str(out), "--output_dir", str(tmp_path / "logs")]
    if tag == "sp":
        cmd.append("--sp-pred")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    want_run = ref["runs"][tag][mode]
    if mode == "predict":
        msgs = [line.split(" - __main__ - ", 1)[1] for line in r.stderr.splitlines() if " - __main__ - " in line]
        body = [m for m in msgs if m in want_run["log"] or any(re.fullmatch(f, m) for f in _LOG_FORMATS)]
        assert len(body) == len(want_run["log"]) and all(re.fullmatch(f, m) for f, m in zip(_LOG_FORMATS, body)), (body, want_run["log"])
        assert any(m.startswith("test performance {") for m in msgs)
    got, want = json.loads(out.read_text()), json.loads(want_run["save_prediction"])
    if want is None:
        assert got is None
        return
    gaps = _margins(ref, npz, tag)
    exempt = sorted(q for q, g in gaps.items() if g < MARGIN)
    print(f"[reader cli {mode} {tag}] exempt (decision margin < {MARGIN}): {exempt}")
    assert set(got) == set(want)
    for key in want:
        for qid in want[key]:
            if qid not in exempt:
                assert got[key][qid] == want[key][qid], (key, qid)
    assert len(exempt) < len(gaps)
