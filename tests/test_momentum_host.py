"""CPU (-m "not gpu"): the host side of momentum training (multihop_dense_retrieval_amd/momentum.py, scripts/train_momentum.py) against
tests/golden/momentum_train_ref.{json,npz}, the reference's own scripts/train_momentum.py --do_train --momentum run on toy assets
(scripts/gen_momentum_train_golden.py): the queue pointer with its truncating enqueue, the run directory's name, the checkpoint files and
their keys; include/mdr_encoder_dropout.h against its binding table and the library; and the refusals the script makes before it touches a
device."""
import ctypes
import importlib
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCRIPT = os.path.join(ROOT, "scripts", "train_momentum.py")


@pytest.fixture(scope="module")
def golden():
    meta = json.load(open(os.path.join(GOLD, "momentum_train_ref.json")))
    z = np.load(os.path.join(GOLD, "momentum_train_ref.npz"))
    return meta, z


def test_fixture_loads_and_is_the_run_the_issue_describes(golden):
    meta, z = golden
    n = meta["n_train_batches"]
    assert meta["k"] == 20 and meta["train_batch"] == 4 and meta["epochs"] == 2 and n == 12
    assert len(meta["loss"]) == len(meta["queue_ptr"]) == len(meta["batch_sizes"]) == n and all(np.isfinite(meta["loss"]))
    assert z["queue0"].shape == (20, 64) or z["queue0"].shape[0] == 20
    assert z["queue0"].dtype == np.float32 and float(np.abs(z["queue0"]).max()) > 0
    for bi in range(n):
        assert z[f"t{bi}.q_input_ids"].shape[0] == meta["batch_sizes"][bi]
        assert z[f"t{bi}.c1_input_ids"].shape == z[f"t{bi}.c1_mask"].shape


def test_memory_bank_replays_the_golden_pointer_sequence(golden):
    """8, 8, then 4 rows: a batch that would pass the end is truncated, and the pointer moves by what was written, modulo k."""
    from multihop_dense_retrieval_amd import criterions
    meta, z = golden
    d = z["queue0"].shape[1]
    bank = criterions.MemoryBank(meta["k"], d)
    bank.queue.copy_(torch.from_numpy(z["queue0"]))
    written = []
    for step, (B, want) in enumerate(zip(meta["batch_sizes"], meta["queue_ptr"])):
        before, ptr = bank.queue.clone(), int(bank.queue_ptr)
        rows = torch.full((2 * B, d), float(step + 1))
        bank.dequeue_and_enqueue(rows)
        assert int(bank.queue_ptr) == want, (step, int(bank.queue_ptr), want)
        n = min(2 * B, meta["k"] - ptr)
        written.append(n)
        assert bool((bank.queue[ptr:ptr + n] == step + 1).all())
        keep = torch.ones(meta["k"], dtype=torch.bool)
        keep[ptr:ptr + n] = False
        assert torch.equal(bank.queue[keep], before[keep]), (step, "rows outside [ptr, ptr + n) were written")
    assert written[:3] == [8, 8, 4] and meta["queue_ptr"][:3] == [8, 16, 0]


def test_run_directory_and_checkpoints_are_the_references(golden):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_momentum
    from multihop_dense_retrieval_amd import retriever
    meta, _ = golden
    args = types.SimpleNamespace(prefix="toy", seed=meta["seed"], train_batch_size=meta["train_batch"], fp16=False, learning_rate=meta["learning_rate"],
                                 weight_decay=0.0, warmup_ratio=0.0, predict_batch_size=4, m=meta["m"], k=meta["k"], temperature=meta["temperature"])
    assert train_momentum.run_name(args) == meta["run_dir"]
    # parsed as the command line gives them (--warmup-ratio 0 and --temperature keep the types the reference's parser gives them)
    from multihop_dense_retrieval_amd.config import train_args
    parsed = train_args(["--prefix", "toy", "--seed", str(meta["seed"]), "--train_batch_size", "4", "--learning_rate", str(meta["learning_rate"]),
                         "--warmup-ratio", "0", "--predict_batch_size", "4", "--m", str(meta["m"]), "--k", str(meta["k"])])
    assert train_momentum.run_name(parsed) == meta["run_dir"]
    ref_files = [f for f in meta["files"] if f.endswith(".pt")]
    assert sorted(train_momentum.CHECKPOINTS_BEST) == sorted(ref_files) and "log.txt" in meta["files"]
    assert train_momentum.CHECKPOINT_LAST not in ref_files  # an addition, as scripts/train_mhop.py adds checkpoint_last.pt
    keys = [k for k, _ in meta["checkpoints"]["checkpoint_q_best.pt"]]
    assert keys == [k for k, _ in meta["checkpoints"]["checkpoint_k_best.pt"]]  # the reference saves encoder_q twice
    cfg = retriever.RobertaConfig(vocab_size=1, hidden_size=64, num_hidden_layers=len({k.split(".")[3] for k in keys if ".layer." in k}))
    ours = sorted(retriever.expected_state_dict_shapes(cfg))  # (the order inside the embeddings is the installed transformers', not 2.11's)
    assert sorted(k for k in keys if not k.endswith("position_ids")) == ours, "checkpoint keys are not RobertaRetriever's"
    assert meta["checkpoint_dtypes"] == ["torch.float32"] or set(meta["checkpoint_dtypes"]) <= {"torch.float32", "torch.int64"}


def test_header_binding_and_library_agree():
    """include/mdr_encoder_dropout.h declares exactly what momentum.SIGNATURES binds and the library exports, apart from every other table."""
    import test_capi_symbols as capi
    from multihop_dense_retrieval_amd import _lib, build, dropout, head, momentum
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdr_encoder_dropout.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert sorted(momentum.SIGNATURES) == declared == ["mdr_encoder_forward_dropout", "mdr_test_embed_ln_dropout", "mdr_test_layernorm_dropout"]
    assert sorted(momentum.EXPORTED_SYMBOLS) == declared
    assert not set(momentum.SIGNATURES) & set(_lib.EXPORTED_SYMBOLS)
    others = [getattr(importlib.import_module("multihop_dense_retrieval_amd." + m), a) for _, m, a, _ in capi.HEADER_TABLES]
    others += [dropout.SIGNATURES] + [getattr(head, "SIGNATURES", {})]
    for table in others:
        assert not set(momentum.SIGNATURES) & set(table)
    for name, (_, args) in momentum.SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args) == proto.count(",") + 1, name
    lib = ctypes.CDLL(build.build_lib())
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mdr_encoder_dropout.h but not exported"
    momentum.lib()  # every signature binds
    assert len(capi.declared_symbols()) == 34  # include/mdr_hip.h did not grow


def test_the_headers_site_formula_is_site_of():
    """site = 1 + (encode * 64 + layer) * 4 + place, as the header states it, against dropout.site_of for every encode, layer and place."""
    from multihop_dense_retrieval_amd import dropout
    text = open(os.path.join(ROOT, "include", "mdr_encoder_dropout.h")).read()
    formula = re.search(r"site = ([^\n]+)", text).group(1).strip()
    places = {int(n): name for n, name in re.findall(r"place (\d)\s+(\w+)", text)}
    assert places == dict(enumerate(dropout.PLACES))
    seen = set()
    for encode in range(dropout.ENCODES):
        for layer in range(dropout.MAX_LAYERS):
            for place, name in places.items():
                if name == "emb" and layer:
                    continue
                got = eval(formula, {"__builtins__": {}}, {"encode": encode, "layer": layer, "place": place})
                assert got == dropout.site_of(encode, layer, name), (encode, layer, name)
                seen.add(got)
    assert 0 not in seen and len(seen) == dropout.ENCODES * (dropout.MAX_LAYERS * 3 + 1)


def run_script(argv):
    return subprocess.run([sys.executable, SCRIPT] + argv, capture_output=True, text=True, timeout=300)


def test_refusals_come_before_the_device(tmp_path):
    logs = tmp_path / "logs"
    r = run_script(["--do_train", "--local_rank", "0", "--model_name", str(tmp_path), "--output_dir", str(logs)])
    assert r.returncode != 0 and "multi-rank momentum training is not built" in r.stderr, r.stderr[-2000:]
    dev = tmp_path / "dev.jsonl"
    dev.write_text("")
    r = run_script(["--do_train", "--model_name", str(tmp_path), "--predict_file", str(dev), "--train_file", str(tmp_path / "none.jsonl"),
                    "--output_dir", str(logs)])
    assert r.returncode != 0 and "--train_file" in r.stderr and "no such file" in r.stderr, r.stderr[-2000:]
    r = run_script(["--do_train", "--model_name", str(tmp_path), "--predict_file", str(dev), "--train_file", str(dev), "--init-retriever",
                    str(tmp_path / "none.pt"), "--output_dir", str(logs)])
    assert r.returncode != 0 and "--init-retriever" in r.stderr and "no such file" in r.stderr, r.stderr[-2000:]
    assert not logs.exists()  # refused before anything is created


def test_train_step_without_momentum_and_train_mhop_with_it_are_refused(tmp_path):
    from multihop_dense_retrieval_amd import momentum
    with pytest.raises(ValueError, match="momentum"):
        momentum.train_step(None, None, types.SimpleNamespace(momentum=False), None, 0)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_mhop.py"), "--do_train", "--momentum", "--model_name", str(tmp_path),
                        "--output_dir", str(tmp_path / "logs")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--momentum is not built" in r.stderr and "scripts/train_momentum.py" in r.stderr, r.stderr[-2000:]
