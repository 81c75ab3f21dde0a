"""GPU (-m gpu): the end-to-end CLI (multihop_dense_retrieval_amd/end2end.py, scripts/end2end.py) on toy assets: the retriever, index and
questions of oracle/gen_cli_golden.build_assets, the corpus with sentences added, the reader of tests/golden/reader_electra_tiny.

1. Its chains are the eval CLI's (--hop2-on-device, beam = topk) for the same questions.
2. The device-assembled reader batch equals QAEvalDataset + qa_collate for the same chains, and the CLI's answers, sp and titles equal
   eval_final's selection over that host-built batch run through the same reader.
3. qa_data.prepare runs at most once per question.
4. On the assets of tests/golden/end2end_ref.* (the reference's own scripts/end2end.py, scripts/gen_end2end_golden.py) the CLI's chains are the
   reference's up to exact ties of its captured path scores, and its answers, sp and titles are the reference's outside a stated margin."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from oracle import gen_cli_golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READER = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny")


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    a = gen_cli_golden.build_assets(str(tmp_path_factory.mktemp("e2e_assets")))
    corpus = {}
    for i, d in enumerate(a["docs"]):
        words = d["text"].split()
        sents = [" ".join(words[j:j + 7]) for j in range(0, len(words), 7)]
        corpus[str(i)] = {"title": d["title"], "text": d["text"], "sents": sents}
    a["e2e_corpus"] = os.path.join(os.path.dirname(a["ckpt"]), "corpus_sents.json")
    with open(a["e2e_corpus"], "w") as f:
        json.dump(corpus, f)
    a["qa_tok"] = transformers.BertTokenizer(os.path.join(READER, "vocab.txt"), do_lower_case=True)
    return a


def _argv(a, topk, batch, sp, save):
    argv = [a["raw"], "--indexpath", a["index"], "--corpus_dict", a["e2e_corpus"], "--retriever_path", a["ckpt"], "--reader_path",
            os.path.join(READER, "ckpt.pt"), "--topk", str(topk), "--batch-size", str(batch), "--retriever-model", a["model_dir"],
            "--reader-model", READER, "--max-q-len", str(gen_cli_golden.MAX_Q_LEN), "--max-q-sp-len", str(gen_cli_golden.MAX_Q_SP_LEN),
            "--num-workers", "0", "--qa-arena-workers", "0", "--save-prediction", save]
    return argv + (["--sp-pred"] if sp else [])


def _reader(sp):
    import types
    from multihop_dense_retrieval_amd import reader
    cfg = transformers.AutoConfig.from_pretrained(READER, local_files_only=True)
    m = reader.QAModel(cfg, types.SimpleNamespace(model_name=READER, sp_pred=sp))
    reader.load_saved(m, os.path.join(READER, "ckpt.pt"), exact=False, map_location="cpu")
    return m.to("cuda").eval()


@pytest.mark.parametrize("topk,batch,sp", [(1, 1, False), (3, 2, True), (4, 5, False)])
def test_end2end_against_eval_cli_chains_and_host_reader_path(assets, tmp_path, topk, batch, sp, monkeypatch, capsys):
    from functools import partial
    from multihop_dense_retrieval_amd import end2end, eval_mhop_retrieval, qa_data
    calls = [0]
    real_prepare = qa_data.prepare

    def counting(*a, **k):
        calls[0] += 1
        return real_prepare(*a, **k)

    monkeypatch.setattr(qa_data, "prepare", counting)
    save = str(tmp_path / "pred.json")
    res = end2end.main(_argv(assets, topk, batch, sp, save), retrieval_tokenizer=assets["tok"], qa_tokenizer=assets["qa_tok"])
    err = capsys.readouterr()
    n_q = len(assets["questions"])
    assert calls[0] <= n_q  # prepare() for the selected chain of each question only
    monkeypatch.setattr(qa_data, "prepare", real_prepare)
    for line in ("Loading trained models...", "Loading corpus...", "Loading index...", "Loading queries...", "Retrieving...", "Reading...", "Answer EM "):
        assert line in err.err, line
    assert "Finishing evaluation in " in err.out
    saved = json.loads(open(save).read())
    assert list(saved) == ["answer", "sp", "titles"] and len(saved["answer"]) == n_q
    assert saved == json.loads(json.dumps(res))

    # 1. chains: those of the eval CLI with beam = topk on the same corpus
    chains = res.chains
    argv = [assets["raw"], assets["index"], assets["e2e_corpus"], assets["ckpt"], "--batch-size", str(batch), "--beam-size", str(topk), "--topk", str(topk),
            "--model-name", assets["model_dir"], "--gpu", "--shared-encoder", "--save-path", str(tmp_path / "paths.jsonl"), "--max-q-len",
            str(gen_cli_golden.MAX_Q_LEN), "--max-q-sp-len", str(gen_cli_golden.MAX_Q_SP_LEN), "--hop2-on-device", "--num-workers", "0"]
    _, recs = eval_mhop_retrieval.main(argv, tokenizer=assets["tok"])
    corpus = json.load(open(assets["e2e_corpus"]))
    assert [[[corpus[str(a)], corpus[str(c)]] for a, c in ch] for ch in chains] == [r["candidate_chains"] for r in recs]

    # 2. device rows == QAEvalDataset + qa_collate; the CLI's answers == eval_final over the host-built batches
    model = _reader(sp)
    tok = assets["qa_tok"]
    from multihop_dense_retrieval_amd import qa_arena
    ar = qa_arena.QAArena.load_or_build(assets["e2e_corpus"], corpus, tok).to("cuda")
    special = qa_arena.special_ids(tok)
    items = [json.loads(line) for line in open(assets["raw"])]
    host_chains = []
    for lo in range(0, n_q, batch):
        qs = items[lo:lo + batch]
        ret = [{"_id": it["_id"], "question": it["question"], "candidate_chains": [[corpus[str(a)], corpus[str(c)]] for a, c in chains[lo + b]]}
               for b, it in enumerate(qs)]
        ds = qa_data.QAEvalDataset(tok, json.loads(json.dumps(ret)), max_seq_len=512, max_q_len=64)
        ref = partial(qa_data.qa_collate, pad_id=tok.pad_token_id)([ds[i] for i in range(len(ds))])
        rows, _ = end2end.assemble_batch(ar, special, end2end.question_ids(tok, [it["question"] for it in qs]), [chains[lo + b] for b in range(len(qs))],
                                         torch.device("cuda", 0))
        for key in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets"):
            assert torch.equal(rows[key].cpu(), ref["net_inputs"][key].to(torch.int64)), (lo, key)
        assert rows["para_offsets"].cpu().tolist() == ref["para_offsets"]
        head = model.decode(ref["net_inputs"], 35)
        lists = {"start": head["start"].tolist(), "end": head["end"].tolist(), "span_score": head["span_score"].float().tolist(),
                 "rank_score": head["rank_score"].view(-1).float().tolist(), "sp_prob": head["sp_prob"].float().tolist() if head["sp_prob"] is not None else None}
        host_chains.extend(qa_data.chain_results(ref, lists, sp, final=True))
    want = qa_data.final_results(host_chains, weight=0.8)
    assert json.loads(json.dumps(want)) == saved
    ems = [qa_data.exact_match_score(saved["answer"][q], it["answer"][0]) for q, it in zip(saved["answer"], items)]
    assert f"Answer EM {np.mean(ems)}" in err.err


def test_end2end_refuses_a_faiss_index_file(assets, tmp_path):
    from multihop_dense_retrieval_amd import end2end
    argv = _argv(assets, 1, 1, False, str(tmp_path / "p.json"))
    argv[argv.index("--indexpath") + 1] = "retrieval/index/wiki_index_hnsw_roberta"
    with pytest.raises(SystemExit, match="FAISS HNSW"):
        end2end.main(argv, retrieval_tokenizer=assets["tok"], qa_tokenizer=assets["qa_tok"])


# The reference ran its reader in fp32 on the CPU; the HIP reader is apex-O1 (fp16 scores). A question is exempt from the answer comparison when
# its decision sits inside that error: the captured runner-up gap of a span (start + end logits) or of the chain selection (0.8 rank + 0.2 span)
# below MARGIN (as tests/test_reader_cli_gpu.py, measured there: logits within 3.9e-3, plus one fp16 rounding of the sum), or when its chains
# differ from the reference's by an exact tie of the captured path scores (duplicate corpus rows).
MARGIN = 0.02


def _reference_margins(z, name, case, max_ans_len=35):
    gaps = []
    for bi in range(case["n_batches"]):
        s, e = torch.from_numpy(z[f"{name}.b{bi}.start_logits"]), torch.from_numpy(z[f"{name}.b{bi}.end_logits"])
        span = s[:, :, None] + e[:, None]
        L = span.size(1)
        band = torch.ones((L, L), dtype=torch.bool).triu(0).tril(max_ans_len)
        flat = span.masked_fill(~band, -float("inf")).flatten(1)
        top2 = flat.topk(2, dim=1).values
        g = float((top2[:, 0] - top2[:, 1]).min())
        sc = sorted((0.8 * float(r) + 0.2 * float(t) for r, t in zip(z[f"{name}.b{bi}.rank_score"].reshape(-1), top2[:, 0])), reverse=True)
        if len(sc) > 1:
            g = min(g, sc[0] - sc[1])
        gaps.append(g)
    return gaps


@pytest.mark.parametrize("name", ["k1_b1", "k3_b2_sp", "k4"])
def test_end2end_against_the_reference_scripts_run(assets, tmp_path, name, capsys):
    from scripts.gen_end2end_golden import corpus_with_sents
    from multihop_dense_retrieval_amd import end2end
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "end2end_ref.json")))
    z = np.load(os.path.join(ROOT, "tests", "golden", "end2end_ref.npz"))
    case = meta["cases"][name]
    corpus = str(tmp_path / "corpus_ref.json")
    with open(corpus, "w") as f:
        json.dump(corpus_with_sents(assets["docs"]), f)
    save = str(tmp_path / "pred.json")
    argv = [assets["raw_small"], "--indexpath", assets["index"], "--corpus_dict", corpus, "--retriever_path", assets["ckpt"], "--reader_path",
            os.path.join(READER, "ckpt.pt"), "--save-prediction", save, "--retriever-model", assets["model_dir"], "--reader-model", READER,
            "--num-workers", "0", "--qa-arena-workers", "0"] + case["flags"]
    res = end2end.main(argv, retrieval_tokenizer=assets["tok"], qa_tokenizer=assets["qa_tok"])
    err = capsys.readouterr().err.split("\n")
    # chains: equal up to exact ties of the captured path scores
    same_chains = []
    for q, (got, want, paths) in enumerate(zip(res.chains, case["chains"], case["paths"])):
        score = {(a, c): s for a, c, s in paths}
        assert all(tuple(g) in score for g in got), (q, got)
        assert [score[tuple(g)] for g in got] == [score[tuple(w)] for w in want], (q, got, want)
        same_chains.append([list(g) for g in got] == want)
    # log lines: the reference's messages (ours adds the arena builds, and loads the corpus before the index)
    for line in case["log"][:-1]:
        assert line in err, line
    got, want = json.loads(open(save).read()), json.loads(case["save_prediction"])
    assert list(got) == list(want) == ["answer", "sp", "titles"]
    gaps = _reference_margins(z, name, case)
    ids = [it["_id"] for it in assets["questions"][:len(case["chains"])]]
    exempt = [qid for qid, g, same in zip(ids, gaps, same_chains) if g < MARGIN or not same]
    print(f"[end2end vs reference {name}] exempt (margin < {MARGIN} or tied chains): {exempt}")
    assert len(exempt) < len(ids)
    for key in want:
        assert set(got[key]) == set(want[key])
        for qid in want[key]:
            if qid not in exempt:
                assert got[key][qid] == want[key][qid], (key, qid)
    if not exempt:
        assert case["log"][-1] in err
