"""GPU (-m gpu): the retriever's dev-set MRR evaluation end to end on the device against tests/golden/mhop_eval_ref.{json,npz} (the reference's
own run of scripts/train_mhop.py --do_predict on toy assets, captured by scripts/gen_mhop_eval_golden.py): RobertaRetriever.forward on the
fixture's batches, the ranks of mdr_inbatch_rank on the device embeddings, and the drop-in CLI in a child process."""
import importlib.util
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("q", "q_sp1", "c1", "c2", "neg_1", "neg_2")
PREFIX = {"q": "q", "q_sp1": "q_sp", "c1": "c1", "c2": "c2", "neg_1": "neg1", "neg_2": "neg2"}
TOL_TINY = (6e-3, 1.2e-3)  # tests/test_encoder_gpu.py TOL["tiny"]: max / mean |err| against the fp32 fixture on the tiny geometry


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mhop_eval_golden", os.path.join(ROOT, "scripts", "gen_mhop_eval_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def setup(golden, tmp_path_factory):
    from multihop_dense_retrieval_amd import retriever
    gen = load_generator()
    a = gen.build_assets(str(tmp_path_factory.mktemp("mhop_assets")))
    geom = a["geom"]
    cfg = retriever.RobertaConfig(vocab_size=geom["vocab"], hidden_size=geom["hidden"], num_hidden_layers=geom["layers"],
                                  num_attention_heads=geom["heads"], intermediate_size=geom["ffn"])
    m = retriever.RobertaRetriever(cfg, None)
    retriever.load_saved(m, a["ckpt"], exact=False, map_location="cpu")
    m.to("cuda").eval()
    meta, npz = golden("mhop_eval_ref.json"), golden("mhop_eval_ref.npz")
    batches = [{k.split(".", 1)[1]: torch.from_numpy(npz[k].astype(np.int64)) for k in npz.files if k.startswith(f"b{bi}.") and ".emb." not in k}
               for bi in range(meta["n_batches"])]
    outs = [m(b) for b in batches]
    return types.SimpleNamespace(gen=gen, a=a, m=m, meta=meta, npz=npz, batches=batches, outs=outs)


def test_forward_matches_the_fixture_and_six_separate_encode_seq_calls(setup):
    worst = (0.0, 0.0)
    for bi, (b, o) in enumerate(zip(setup.batches, setup.outs)):
        assert list(o) == ["c1", "c2", "neg_1", "neg_2", "q", "q_sp1"]
        for k in KEYS:
            err = np.abs(o[k].cpu().numpy() - setup.npz[f"b{bi}.emb.{k}"])
            worst = (max(worst[0], err.max()), max(worst[1], err.mean()))
            assert err.max() <= TOL_TINY[0] and err.mean() <= TOL_TINY[1], (bi, k, err.max(), err.mean())
            alone = setup.m.encode_seq(b[f"{PREFIX[k]}_input_ids"], b[f"{PREFIX[k]}_mask"])
            assert torch.equal(alone, o[k]), (bi, k)
    print(f"embedding error against the fixture: max {worst[0]:.2e}, mean {worst[1]:.2e}")


def device_rrs(setup, fp16):
    from multihop_dense_retrieval_amd import criterions
    return [criterions.mhop_eval(o, types.SimpleNamespace(fp16=fp16)) for o in setup.outs]


def decided_masks(setup, fp16):
    """gen.decided on the FIXTURE's scores with the elementwise embedding error measured here, per matrix and batch. Under --fp16 the operands
    are rounded to fp16 (relative 2^-11 per element) and so is every score (2^-11 of its magnitude covers the half ulp twice over)."""
    masks = []
    for bi, o in enumerate(setup.outs):
        ref = {k: setup.npz[f"b{bi}.emb.{k}"] for k in KEYS}
        err = {k: float(np.abs(o[k].cpu().numpy() - ref[k]).max()) for k in KEYS}
        slack = 0.0
        if fp16:
            err = {k: err[k] + 2.0 ** -11 * float(np.abs(ref[k]).max()) for k in KEYS}
            slack = 2.0 ** -11 * max(float(np.abs(s[np.isfinite(s)]).max()) for s, _, _ in setup.gen.score_matrices(ref))
        masks.append(setup.gen.decided(ref, err, slack))
    return masks


def test_device_ranks_equal_the_reference_where_the_fixture_decides(setup):
    got = device_rrs(setup, fp16=False)
    masks = decided_masks(setup, fp16=False)
    n = sum(m.size for m in masks)
    excluded = sum(int((~m).sum()) for m in masks)
    print(f"ranks excluded (target within the measured embedding error x |row| of another score): {excluded} of {n} ({excluded / n:.1%})")
    assert excluded / n <= 0.10
    for bi, (g, m) in enumerate(zip(got, masks)):
        for h, key in enumerate(("rrs_1", "rrs_2")):
            ref = setup.meta[key][bi]
            for i, (x, y) in enumerate(zip(g[key], ref)):
                if m[h, i]:
                    assert x == y, (bi, key, i, x, y)


def run_cli(setup, extra):
    argv = [sys.executable, os.path.join(ROOT, "scripts", "train_mhop.py")] + setup.gen.cli_argv(setup.a, extra)
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln.split(" - __main__ - ", 1)[1] for ln in r.stderr.split("\n") if " - __main__ - " in ln]
    return lines


def test_cli_prints_the_reference_log_lines(setup):
    from multihop_dense_retrieval_amd import criterions
    lines = run_cli(setup, [])
    got = device_rrs(setup, fp16=False)
    exp_lines, perf = criterions.predict_summary(sum((g["rrs_1"] for g in got), []), sum((g["rrs_2"] for g in got), []))
    assert f"Num of dev batches: {setup.meta['n_batches']}" in lines
    assert lines[-4:-1] == exp_lines and lines[-1] == f"test performance {perf}"
    ref = [ln.split(" - __main__ - ", 1)[1] for ln in setup.meta["log"]]
    assert lines[-4] == ref[-4]  # `evaluated 24 examples...`
    for mine, theirs in zip(lines[-3:-1], ref[-3:-1]):  # MRR-1 / MRR-2: equal up to the excluded ranks, each of which moves a mean of n by < 1 / n
        masks = decided_masks(setup, fp16=False)
        n = sum(m.shape[1] for m in masks)
        hop = 0 if mine.startswith("MRR-1") else 1
        slack = sum(int((~m[hop]).sum()) for m in masks) / n
        assert mine.split(":")[0] == theirs.split(":")[0]
        assert abs(float(mine.split(": ")[1]) - float(theirs.split(": ")[1])) <= slack + 1e-12, (mine, theirs, slack)


def test_cli_fp16_completes_and_stays_within_the_exclusion_set(setup, tmp_path):
    r32 = run_cli(setup, [])
    before = set(os.listdir(tmp_path))
    argv = [sys.executable, os.path.join(ROOT, "scripts", "train_mhop.py")] + setup.gen.cli_argv(setup.a, ["--fp16", "--output_dir", str(tmp_path / "logs")])
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]
    assert set(os.listdir(tmp_path)) == before  # no dated output directory, log.txt or TensorBoard files for --do_predict
    r16 = [ln.split(" - __main__ - ", 1)[1] for ln in r.stderr.split("\n") if " - __main__ - " in ln]
    masks = decided_masks(setup, fp16=True)
    n = sum(m.shape[1] for m in masks)
    for hop, (a16, a32) in enumerate(zip(r16[-3:-1], r32[-3:-1])):
        assert re.fullmatch(rf"MRR-{hop + 1}: [0-9.e-]+", a16)
        slack = sum(int((~m[hop]).sum()) for m in masks) / n
        d = abs(float(a16.split(": ")[1]) - float(a32.split(": ")[1]))
        print(f"{a16} (fp16) vs {a32} (fp32): |diff| {d:.4f}, undecided share under fp16 rounding {slack:.3f}")
        assert d <= slack + 1e-12
    # in process: the fp16 ranks equal the fp32 ranks wherever the fixture decides under the fp16 allowance
    g16, g32 = device_rrs(setup, True), device_rrs(setup, False)
    for a, b, m in zip(g16, g32, masks):
        for h, key in enumerate(("rrs_1", "rrs_2")):
            assert all(x == y for x, y, ok in zip(a[key], b[key], m[h]) if ok)
