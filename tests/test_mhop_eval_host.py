"""CPU (-m "not gpu"): the host side of the retriever's dev-set MRR evaluation (scripts/train_mhop.py --do_predict) against
tests/golden/mhop_eval_ref.{json,npz}, which scripts/gen_mhop_eval_golden.py captured from the reference's own run on toy assets:
the data path, the host statement of the rank formula, the log lines, the loss value, the flags, and the C ABI's binding table."""
import ast
import glob
import importlib.util
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("q", "q_sp1", "c1", "c2", "neg_1", "neg_2")


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mhop_eval_golden", os.path.join(ROOT, "scripts", "gen_mhop_eval_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("mhop_eval_ref.json"), golden("mhop_eval_ref.npz")


def fixture_embeddings(npz, bi):
    return {k: torch.from_numpy(npz[f"b{bi}.emb.{k}"]) for k in KEYS}


def test_data_path_reproduces_the_reference_batches(fixture, tmp_path):
    """MhopDataset + mhop_collate give the reference's collated tensors exactly: every key, including the order of the comparison questions'
    positives under random.seed(--seed) (items read once, in dataset order, as a DataLoader with num_workers 0 does)."""
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import mhop_data
    meta, npz = fixture
    gen = load_generator()
    a = gen.build_assets(str(tmp_path))
    assert a["samples"] == meta["samples"]
    random.seed(meta["seed"])
    ds = mhop_data.MhopDataset(a["tok"], a["dev"], meta["max_q_len"], meta["max_q_sp_len"], meta["max_c_len"])
    batches = list(DataLoader(ds, batch_size=meta["batch"], collate_fn=mhop_data.mhop_collate, num_workers=0))
    assert len(batches) == meta["n_batches"]
    names = sorted(k.split(".", 1)[1] for k in npz.files if k.startswith("b0.") and ".emb." not in k)
    assert len(names) == 12
    truncated_c = truncated_qsp = 0
    for bi, b in enumerate(batches):
        assert sorted(b) == names
        for k in names:
            assert b[k].dtype == torch.int64
            assert np.array_equal(b[k].numpy(), npz[f"b{bi}.{k}"]), (bi, k)
        truncated_c += int((b["c1_mask"].sum(1) == meta["max_c_len"]).sum())
        truncated_qsp += int((b["q_sp_mask"].sum(1) == meta["max_q_sp_len"]).sum())
    assert truncated_c >= 1 and truncated_qsp >= 1  # the fixture really cuts a passage and a question + passage pair
    # the shuffle matters: with another seed the comparison questions' positives come out in another order somewhere
    random.seed(meta["seed"] + 1)
    ds2 = mhop_data.MhopDataset(a["tok"], a["dev"], meta["max_q_len"], meta["max_q_sp_len"], meta["max_c_len"])
    other = list(DataLoader(ds2, batch_size=meta["batch"], collate_fn=mhop_data.mhop_collate, num_workers=0))
    assert any(o["c1_input_ids"].shape != b["c1_input_ids"].shape or not torch.equal(o["c1_input_ids"], b["c1_input_ids"]) for o, b in zip(other, batches))
    with pytest.raises(NotImplementedError, match="training is not supported"):
        mhop_data.MhopDataset(a["tok"], a["dev"], 10, 10, 10, train=True)


def test_host_formula_reproduces_the_reference_ranks_and_log_lines(fixture):
    from multihop_dense_retrieval_amd import criterions
    meta, npz = fixture
    rrs_1, rrs_2 = [], []
    for bi in range(meta["n_batches"]):
        r = criterions.mhop_eval_host(fixture_embeddings(npz, bi), fp16=False)
        assert r["rrs_1"] == meta["rrs_1"][bi] and r["rrs_2"] == meta["rrs_2"][bi], bi
        rrs_1 += r["rrs_1"]
        rrs_2 += r["rrs_2"]
    lines, perf = criterions.predict_summary(rrs_1, rrs_2)
    ref_lines = [ln.split(" - __main__ - ", 1)[1] for ln in meta["log"]]
    assert ref_lines[-4:-1] == lines  # `evaluated n examples...`, `MRR-1: ..`, `MRR-2: ..`: the floats through the reference's own formatting
    assert ref_lines[-1] == f"test performance {perf}" and meta["test_performance"] == f"{perf}"
    assert f"Num of dev batches: {meta['n_batches']}" in ref_lines
    assert 0.1 < perf["mrr_avg"] < 0.95  # not a degenerate fixture


def test_tie_rule_is_the_stable_descending_sort():
    from multihop_dense_retrieval_amd import criterions
    s = np.array([[1.0, 3.0, 3.0, 2.0, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0], [np.nan, 1.0, 2.0, 0.0, 0.0], [5.0, -np.inf, 5.0, np.inf, 1.0]])
    t = np.array([2, 3, 0, 2])
    assert criterions.stable_ranks(s, t).tolist() == [2, 4, 5, 3]
    for row, tt in zip(s[[0, 1, 3]], t[[0, 1, 3]]):
        order = np.argsort(-row, kind="stable")
        assert criterions.stable_ranks(row[None], np.array([tt]))[0] == 1 + int(np.nonzero(order == tt)[0][0])
    # fp16 scores tie where fp32 scores do not: 2048 + 1 is not an fp16 number
    o = {k: torch.zeros(1, 32) for k in KEYS}
    o["q"][0, :2] = torch.tensor([1.0, 1.0])
    o["q_sp1"] = o["q"].clone()
    o["c1"][0, :2] = torch.tensor([2048.0, 0.0])  # target of hop 1: 2048
    o["neg_1"][0, :2] = torch.tensor([2048.0, 1.0])  # 2049 in fp32, 2048 in fp16 (ties, but comes after the target)
    o["c2"][0, :2] = torch.tensor([2048.0, 1.0])  # target of hop 2 (column 1): 2049 -> 2048 in fp16, tied with column 0 before it
    assert criterions.mhop_eval_host(o, fp16=False) == {"rrs_1": [1 / 2], "rrs_2": [1 / 1]}
    assert criterions.mhop_eval_host(o, fp16=True) == {"rrs_1": [1 / 1], "rrs_2": [1 / 2]}


def test_loss_value_matches_the_reference(fixture):
    """mhop_loss_value (host) on the fixture's embeddings against the reference's mhop_loss on the same tensors. Both are fp32 cross entropies of
    the same fp32 scores: per row, logsumexp - target carries a few ulps of the larger of the two magnitudes (exp, log, the subtraction: <= 4
    ulps of max(|lse|, |t|) <= 4 * 2^-23 * that magnitude), and the mean of B such terms plus the sum of the two hops add B + 1 more roundings
    of numbers no larger than that. Bound: (4 + B + 1) * 2^-23 * (max magnitude of hop 1 + of hop 2)."""
    from multihop_dense_retrieval_amd import criterions
    meta, npz = fixture
    for bi in range(meta["n_batches"]):
        o = fixture_embeddings(npz, bi)
        s1, s2 = criterions.host_scores(o, False)
        B = s1.shape[0]
        mag = sum(float(torch.maximum(torch.logsumexp(s.double(), dim=1).abs(), s.double()[torch.arange(B), torch.arange(B) + h * B].abs()).max())
                  for h, s in enumerate((s1, s2)))
        tol = (4 + B + 1) * 2.0 ** -23 * mag
        got = criterions.mhop_loss_value(o, fp16=False)
        print(f"batch {bi}: loss {got!r} reference {meta['mhop_loss'][bi]!r} bound {tol:.3e}")
        assert abs(got - meta["mhop_loss"][bi]) <= tol


def test_readme_training_argv_parses_and_do_train_exits():
    from multihop_dense_retrieval_amd import config
    argv = ("--do_train --prefix run1 --predict_batch_size 3000 --model_name roberta-base --train_batch_size 150 --learning_rate 2e-5 --fp16 "
            "--train_file train.json --predict_file dev.json --seed 16 --eval-period -1 --max_c_len 300 --max_q_len 70 --max_q_sp_len 350 "
            "--shared-encoder --warmup-ratio 0.1").split()
    a = config.train_args(argv)
    assert (a.do_train, a.predict_batch_size, a.train_batch_size, a.learning_rate, a.fp16, a.seed, a.eval_period, a.max_c_len, a.max_q_len,
            a.max_q_sp_len, a.shared_encoder, a.warmup_ratio, a.prefix) == (True, 3000, 150, 2e-5, True, 16, -1, 300, 70, 350, True, 0.1, "run1")
    d = config.train_args([])
    assert (d.weight_decay, d.temperature, d.output_dir, d.adam_epsilon, d.num_train_epochs, d.save_checkpoints_steps, d.iterations_per_loop,
            d.accumulate_gradients, d.seed, d.gradient_accumulation_steps, d.max_grad_norm, d.stop_drop, d.use_adam, d.num_workers) == \
        (0.0, 1, "./logs", 1e-8, 50, 20000, 1000, 1, 3, 1, 2.0, 0, False, 30)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_mhop.py")] + argv, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "training is not supported" in r.stderr


def test_retriever_forward_is_six_encode_seq_calls():
    """RobertaRetriever(batch) no longer raises: it maps mhop_collate's keys to the reference's six outputs, one encode_seq each."""
    from multihop_dense_retrieval_amd import retriever
    m = retriever.RobertaRetriever(retriever.RobertaConfig(), None)
    calls = []
    m.encode_seq = lambda ids, mask, lane=0: calls.append((ids, mask)) or ids
    batch = {f"{k}_{s}": f"{k}.{s}" for k in ("q", "q_sp", "c1", "c2", "neg1", "neg2") for s in ("input_ids", "mask")}
    out = m(batch)
    assert out == {"q": "q.input_ids", "q_sp1": "q_sp.input_ids", "c1": "c1.input_ids", "c2": "c2.input_ids", "neg_1": "neg1.input_ids", "neg_2": "neg2.input_ids"}
    assert calls == [(f"{k}.input_ids", f"{k}.mask") for k in ("c1", "c2", "neg1", "neg2", "q", "q_sp")]


def test_fixture_is_data_and_the_generator_stays_outside_the_package(fixture):
    meta, npz = fixture
    assert meta["undecided_share_at_assumed_err"] <= 0.10
    assert sum(s["type"] == "comparison" for s in meta["samples"]) >= 4 and any(not s["question"].endswith("?") for s in meta["samples"])
    for k in npz.files:
        assert npz[k].dtype in (np.int32, np.float32), k
    for path in sorted(glob.glob(os.path.join(ROOT, "multihop_dense_retrieval_amd", "**", "*.py"), recursive=True)) + [os.path.join(ROOT, "scripts", "train_mhop.py")]:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            names = []
            if isinstance(node, ast.Import):
                names = [x.name for x in node.names]
            elif isinstance(node, ast.ImportFrom):
                names = [node.module or ""]
            elif isinstance(node, ast.Constant) and isinstance(node.value, str) and re.fullmatch(r"[\w./]*gen_mhop_eval_golden(\.py)?", node.value):
                names = [node.value]
            for n in names:
                assert "gen_mhop_eval_golden" not in n and not (n == "oracle" or n.startswith("oracle.")), f"{path} reaches the generator / the checker: {n}"
    for size in (os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in ("mhop_eval_ref.json", "mhop_eval_ref.npz")):
        assert size < 1 << 20
    json.dumps(meta)  # plain data
