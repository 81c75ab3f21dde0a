"""CPU (-m "not gpu"): the answer reader's host side -- its C ABI (include/mdr_reader.h) against the binding table and the library,
the checkpoint schema against the reference QAModel's, the refusal of model families the kernels do not compute, and the span
search's torch restatement (the formula of scripts/train_qa.py predict(), used by the GPU tests as the bit-exact yardstick) against
an independent walk over the band."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_struct_matches_header():
    from multihop_dense_retrieval_amd import reader
    text = open(os.path.join(ROOT, "include", "mdr_reader.h")).read()
    body = re.search(r"typedef struct mdr_reader_config \{(.*?)\} mdr_reader_config;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split()[1:] for f in f.split(",") if f.strip()]
    assert fields == [f for f, _ in reader.ReaderConfig._fields_]
    body = re.search(r"typedef struct mdr_reader_outputs \{(.*?)\} mdr_reader_outputs;", text, re.S).group(1)
    names = re.findall(r"\*\s*(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f for f, _ in reader.ReaderOutputs._fields_]


def _electra_config(**kw):
    transformers = pytest.importorskip("transformers")
    base = dict(vocab_size=300, hidden_size=128, embedding_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
                max_position_embeddings=512, type_vocab_size=2)
    base.update(kw)
    return transformers.ElectraConfig(**base)


@pytest.mark.parametrize("sp_pred", [False, True])
def test_state_dict_schema_is_the_reference_qamodels(sp_pred):
    """Key set and shapes of qa_model.py's QAModel.state_dict(): the HF ElectraModel's parameters under `encoder.`, BertPooler's under
    `pooler.`, the heads (buffers such as position_ids are not weights and are ignored by load_saved(exact=False))."""
    transformers = pytest.importorskip("transformers")
    from multihop_dense_retrieval_amd import reader
    cfg = _electra_config()
    enc = transformers.ElectraModel(cfg)
    ref = {"encoder." + k: tuple(p.shape) for k, p in enc.named_parameters()}
    H = cfg.hidden_size
    ref.update({"pooler.dense.weight": (H, H), "pooler.dense.bias": (H,), "qa_outputs.weight": (2, H), "qa_outputs.bias": (2,),
                "rank.weight": (1, H), "rank.bias": (1,)})
    if sp_pred:
        ref.update({"sp.weight": (1, H), "sp.bias": (1,)})
    m = reader.QAModel(cfg, types.SimpleNamespace(model_name="google/electra-base-discriminator", sp_pred=sp_pred))
    assert {k: tuple(v) for k, v in m.state_dict().items()} == ref


def test_bert_family_pooler_lives_in_the_encoder():
    transformers = pytest.importorskip("transformers")
    from multihop_dense_retrieval_amd import reader
    cfg = transformers.BertConfig(vocab_size=300, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)
    enc = transformers.BertModel(cfg)
    m = reader.QAModel(cfg, types.SimpleNamespace(model_name="bert-base-uncased", sp_pred=False))
    keys = set(m.state_dict())
    assert {"encoder." + k for k, _ in enc.named_parameters()} <= keys
    assert "encoder.pooler.dense.weight" in keys and "pooler.dense.weight" not in keys


def test_unsupported_families_fail_by_name():
    from multihop_dense_retrieval_amd import reader
    with pytest.raises(NotImplementedError, match="embeddings_project"):
        reader.QAModel(_electra_config(embedding_size=64), types.SimpleNamespace(model_name="google/electra-small-discriminator", sp_pred=True))
    with pytest.raises(NotImplementedError, match="RoBERTa"):
        reader.QAModel(_electra_config(), types.SimpleNamespace(model_name="roberta-large", sp_pred=True))
    with pytest.raises(NotImplementedError, match="SpanBERT"):
        reader.QAModel(_electra_config(), types.SimpleNamespace(model_name="SpanBERT/spanbert-large-cased", sp_pred=True))


def test_load_saved_semantics(tmp_path):
    """utils.load_saved: a `module.` prefix is stripped; exact=False drops unknown keys; a missing key raises."""
    from multihop_dense_retrieval_amd import reader
    m = reader.QAModel(_electra_config(), types.SimpleNamespace(model_name="google/electra-base-discriminator", sp_pred=True))
    sd = {"module." + k: torch.zeros(shp) for k, shp in m.state_dict().items()}
    sd["module.extra.weight"] = torch.zeros(3)
    p = str(tmp_path / "ckpt.pt")
    torch.save(sd, p)
    reader.load_saved(m, p, exact=False)
    assert set(m._pending) == set(m.state_dict())
    with pytest.raises(RuntimeError, match="Unexpected"):
        reader.load_saved(m, p, exact=True)
    del sd["module.sp.weight"]
    torch.save(sd, p)
    with pytest.raises(RuntimeError, match="sp.weight"):
        reader.load_saved(m, p, exact=False)


def test_reader_has_no_cpu_fallback():
    from multihop_dense_retrieval_amd import reader
    m = reader.QAModel(_electra_config(), types.SimpleNamespace(model_name="google/electra-base-discriminator", sp_pred=False))
    with pytest.raises(RuntimeError):
        m.to("cpu")


# ---- span search ------------------------------------------------------------------------------------------------------------------
def band_walk(start, end, max_ans_len, dtype):
    """Independent restatement: visit every in-band cell in row-major order, keep the first strict maximum. In fp16 the out-of-band
    cells are -inf (-1e10 does not survive .type_as), so they never beat the in-band cell (0, 0); in fp32 they are -1e10, which does
    beat an all -inf band -- that case is excluded by the callers of the fp32 variant."""
    B, L = start.shape
    res = []
    for b in range(B):
        best = None
        for s in range(L):
            for e in range(s, min(L - 1, s + max_ans_len) + 1):
                v = (np.asarray(start[b, s], dtype) + np.asarray(end[b, e], dtype)).astype(dtype)
                if best is None or v > best[0]:
                    best = (v, s, e)
        res.append(best)
    return res


def _logits(rng, B, L, kind, dtype):
    if kind == "ties":  # few distinct values: exact ties everywhere
        x = rng.integers(-3, 3, size=(2, B, L)).astype(np.float32) * 0.5
    else:
        x = rng.normal(0, 4, size=(2, B, L)).astype(np.float32)
    mask = rng.random((B, L)) < 0.3
    mask[:, 0] = True  # CLS-like position outside the paragraph
    x[:, mask] = -np.inf
    return torch.from_numpy(x[0]).to(dtype), torch.from_numpy(x[1]).to(dtype)


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("max_ans_len", [0, 1, 5, 35])
def test_span_reference_formula_matches_band_walk_fp16(kind, max_ans_len):
    from multihop_dense_retrieval_amd import reader
    rng = np.random.default_rng(max_ans_len * 7 + len(kind))
    for B, L in ((1, 1), (3, 9), (4, 40)):
        s, e = _logits(rng, B, L, kind, torch.float16)
        if B == 4:
            s[3] = -float("inf")  # a fully masked row: (0, 0) with -inf
        st, en, sc = reader.span_search_reference(s, e, max_ans_len)
        for b, (v, s0, e0) in enumerate(band_walk(s.float().numpy(), e.float().numpy(), max_ans_len, np.float16)):
            assert (int(st[b]), int(en[b])) == (s0, e0), (b, L, max_ans_len)
            assert np.float16(sc[b].item()) == v or (np.isinf(v) and np.isinf(sc[b].item()))


@pytest.mark.parametrize("kind", ["random", "ties"])
def test_span_reference_formula_matches_band_walk_fp32(kind):
    from multihop_dense_retrieval_amd import reader
    rng = np.random.default_rng(11)
    for max_ans_len in (0, 3, 30):
        s, e = _logits(rng, 5, 33, kind, torch.float32)
        st, en, sc = reader.span_search_reference(s, e, max_ans_len)
        for b, (v, s0, e0) in enumerate(band_walk(s.numpy(), e.numpy(), max_ans_len, np.float32)):
            if np.isinf(v):
                continue
            assert (int(st[b]), int(en[b]), np.float32(sc[b].item())) == (s0, e0, v)


def test_fp16_ties_follow_torch_first_index():
    """Equal fp16 sums: the row-major-first (s, e) wins. 2048 + 1 rounds to 2048 in fp16, so an fp16 sum ties where fp32 does not."""
    from multihop_dense_retrieval_amd import reader
    t = lambda v, dt=torch.float16: torch.tensor([v], dtype=dt)  # noqa: E731
    st, en, sc = reader.span_search_reference(t([0.0, 1.0, 1.0, 0.0]), t([0.0, 1.0, 1.0, 0.0]), 1)
    assert (int(st[0]), int(en[0]), float(sc[0])) == (1, 1, 2.0)  # (1, 1), (1, 2) and (2, 2) all sum to 2
    st, en, sc = reader.span_search_reference(t([2048.0, -float("inf")]), t([0.0, 1.0]), 1)
    assert (int(st[0]), int(en[0]), float(sc[0])) == (0, 0, 2048.0)
    st, en, sc = reader.span_search_reference(t([2048.0, -float("inf")], torch.float32), t([0.0, 1.0], torch.float32), 1)
    assert (int(st[0]), int(en[0]), float(sc[0])) == (0, 1, 2049.0)
