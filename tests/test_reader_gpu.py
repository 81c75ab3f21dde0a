"""GPU (-m gpu): the answer reader (include/mdr_reader.h) against restatements of the reference on the device.

1. The span search kernel, on caller-given fp16 logits, returns start, end and span_score BIT-IDENTICAL to predict()'s own [B, L, L]
   formulation (reader.span_search_reference, itself checked against an independent band walk in tests/test_reader_host.py):
   random, tie-heavy and fully masked rows, max_ans_len in {0, 1, 30, 35, L}, L up to 512, B = 1 and ragged batches.
2. The full forward (ELECTRA embedding, every layer over every token, heads) against HF transformers' ElectraModel / BertModel in fp64 on
   the device plus the heads of qa_model.py in fp64, with random weights of O(1) sub-layer outputs (as oracle/seeded.py does for the
   retrieval encoder). The bar is fp16-operand noise (apex O1, the regime of the README's --fp16 runs) relative to the logits' scale;
   the span outputs of decode() must be bit-identical to predict()'s formula applied to the kernel's own logits, and the masked
   positions exactly -inf."""
import types

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")

from multihop_dense_retrieval_amd import reader  # noqa: E402

DEV = "cuda"


def _logits(g, B, L, kind):
    if kind == "ties":
        x = torch.randint(-3, 3, (2, B, L), generator=g).float() * 0.5
    elif kind == "big":  # sums that round in fp16 (spacing 2 .. 8 above 2048)
        x = 2048 + torch.randint(0, 64, (2, B, L), generator=g).float()
    else:
        x = torch.randn((2, B, L), generator=g) * 4
    masked = torch.rand((B, L), generator=g) < 0.3
    masked[:, 0] = True
    x[:, masked] = -float("inf")
    return x[0].half().to(DEV), x[1].half().to(DEV)


@pytest.mark.parametrize("L", [1, 2, 63, 128, 300, 512])
@pytest.mark.parametrize("kind", ["random", "ties", "big"])
def test_span_kernel_is_bit_identical_to_the_reference_formula(L, kind):
    g = torch.Generator().manual_seed(L * 3 + len(kind))
    for B in (1, 5, 37):
        s, e = _logits(g, B, L, kind)
        if B > 1:
            s[B // 2] = -float("inf")  # a fully masked row: (0, 0), -inf
        for mal in sorted({0, 1, 30, 35, L}):
            got = reader.span_search(s, e, mal)
            ref = reader.span_search_reference(s, e, mal)
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (B, L, mal)
            assert torch.equal(got[2].view(torch.int16), ref[2].view(torch.int16)), (B, L, mal)


def _random_state_dict(config, family, sp_pred, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = reader.expected_state_dict_shapes(config, family, sp_pred)
    sd = {}
    for k, shp in shapes.items():
        if k.endswith("LayerNorm.weight"):
            sd[k] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        elif "embeddings" in k:
            sd[k] = 0.5 * torch.randn(shp, generator=g)
        else:
            sd[k] = (1.5 / shp[1] ** 0.5) * torch.randn(shp, generator=g)
    return sd


def _batch(config, lens, L, n_sent, seed):
    """qa_collate-shaped inputs: [CLS] q [SEP] paragraph [SEP], right padding, token types 1 after the first [SEP], paragraph_mask over
    the paragraph without its final [SEP], sentence markers inside the paragraph (0 = padding)."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    ids = torch.zeros((B, L), dtype=torch.int64)
    mask = torch.zeros_like(ids)
    tt = torch.zeros_like(ids)
    pm = torch.zeros_like(ids)
    so = torch.zeros((B, n_sent), dtype=torch.int64)
    for b, n in enumerate(lens):
        q = max(1, min(n // 4, 30))
        ids[b, :n] = torch.randint(5, config.vocab_size, (n,), generator=g)
        mask[b, :n] = 1
        tt[b, q + 2:n] = 1
        pm[b, q + 2:n - 1] = 1
        k = min(n_sent - b % 2, max(0, n - q - 3))
        if k > 0:
            so[b, :k] = torch.sort(torch.randperm(n - q - 3, generator=g)[:k] + q + 2).values
    return {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt, "paragraph_mask": pm, "sent_offsets": so}


def _reference(config, family, sd, batch, sp_pred):
    """qa_model.py QAModel.forward in fp64 on the device: HF ElectraModel / BertModel (transformers, eager attention) + the heads."""
    cls = transformers.ElectraModel if family == "electra" else transformers.BertModel
    kw = {} if family == "electra" else {"add_pooling_layer": True}
    enc = cls(config, **kw).to(DEV).double().eval()
    missing, unexpected = enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, strict=False)
    assert not [m for m in missing if "position_ids" not in m] and not unexpected, (missing, unexpected)
    W = {k: v.to(DEV).double() for k, v in sd.items() if not k.startswith("encoder.") or "pooler" in k}
    b = {k: v.to(DEV) for k, v in batch.items()}
    with torch.no_grad():
        h = enc(b["input_ids"], attention_mask=b["attention_mask"], token_type_ids=b["token_type_ids"])[0]
        lo = h @ W["qa_outputs.weight"].T + W["qa_outputs.bias"]
        neg = b["paragraph_mask"].ne(1)
        start, end = lo[..., 0].masked_fill(neg, -float("inf")), lo[..., 1].masked_fill(neg, -float("inf"))
        pk = "pooler.dense." if family == "electra" else "encoder.pooler.dense."
        pooled = torch.tanh(h[:, 0] @ W[pk + "weight"].T + W[pk + "bias"])
        rank = pooled @ W["rank.weight"].T + W["rank.bias"]
        sp = None
        if sp_pred:
            rep = torch.gather(h, 1, b["sent_offsets"].unsqueeze(2).expand(-1, -1, h.size(-1)))
            sp = (rep @ W["sp.weight"].T + W["sp.bias"]).squeeze(2)
    return {"start_logits": start, "end_logits": end, "rank_score": rank, "sp_score": sp}


def _model(config, family, sd, sp_pred):
    name = "google/electra-test-discriminator" if family == "electra" else "bert-test-uncased"
    m = reader.QAModel(config, types.SimpleNamespace(model_name=name, sp_pred=sp_pred))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _check(m, ref, batch, tol, label, max_ans_len=30):
    out = m(batch)
    dec = m.decode(batch, max_ans_len, with_logits=True)
    finite = torch.isfinite(ref["start_logits"])
    scale = ref["start_logits"][finite].abs().mean().item()
    errs = {}
    for k in ("start_logits", "end_logits"):
        got, want = out[k], ref[k]
        assert got.dtype == torch.float16
        assert torch.equal(torch.isinf(got), torch.isinf(want)), k  # -inf exactly where the reference masks
        errs[k] = (got.double() - want)[finite].abs().max().item() / scale
        assert torch.equal(dec[k].view(torch.int16), got.view(torch.int16)), k  # the fused path computes the same logits
    errs["rank"] = (out["rank_score"].double() - ref["rank_score"]).abs().max().item() / max(ref["rank_score"].abs().mean().item(), 1e-3)
    assert out["rank_score"].shape == ref["rank_score"].shape
    if ref["sp_score"] is not None:
        errs["sp"] = (out["sp_score"].double() - ref["sp_score"]).abs().max().item() / max(ref["sp_score"].abs().mean().item(), 1e-3)
        so = batch["sent_offsets"].to(DEV)
        want_prob = out["sp_score"].float().masked_fill(so.eq(0), float("-inf")).half().sigmoid()
        assert torch.equal(dec["sp_prob"].view(torch.int16), want_prob.view(torch.int16))  # predict()'s mask + fp16 sigmoid, exactly
    print(f"[reader {label}] max |err| / mean |logit|: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= tol, (label, k, v, tol)
    s, e, sc = reader.span_search_reference(out["start_logits"], out["end_logits"], max_ans_len)
    assert torch.equal(dec["start"], s) and torch.equal(dec["end"], e) and torch.equal(dec["span_score"].view(torch.int16), sc.view(torch.int16))
    return errs


def _electra(hidden, layers, ffn, vocab=1000):
    return transformers.ElectraConfig(vocab_size=vocab, hidden_size=hidden, embedding_size=hidden, num_hidden_layers=layers,
                                      num_attention_heads=hidden // 64, intermediate_size=ffn, max_position_embeddings=512, type_vocab_size=2,
                                      layer_norm_eps=1e-12, attn_implementation="eager")


# max |err| relative to the reference's mean |output|. Measured on an MI355X, recorded in profiles/reader_bench.md ("Parity error"): 1- and 2-layer geometries
# (hidden 128 / 256, every residual mode, BERT too) at most 7.7e-3 on the logits and 6.9e-3 on rank / sp; ELECTRA-large (24 layers)
# 2.3e-2 at L = 384 and 4.6e-2 at L = 512 on the logits, <= 4.6e-3 on rank / sp (the error grows with depth, as the encoder's does).
TOL_TINY, TOL_LARGE = 0.015, 0.08


@pytest.mark.parametrize("sp_pred", [True, False])
@pytest.mark.parametrize("residual_fp32", [2, 1, 0])
def test_tiny_electra_reader_matches_fp64_reference(sp_pred, residual_fp32):
    cfg = _electra(256, 2, 1024)
    sd = _random_state_dict(cfg, "electra", sp_pred, seed=3)
    batch = _batch(cfg, [200, 77, 512, 1, 130], 512, 8, seed=4)
    ref = _reference(cfg, "electra", sd, batch, sp_pred)
    m = reader.QAModel(cfg, types.SimpleNamespace(model_name="google/electra-test-discriminator", sp_pred=sp_pred))
    m.residual_fp32 = residual_fp32
    m.load_state_dict(sd)
    m.to(DEV)
    _check(m, ref, batch, TOL_TINY, f"tiny sp={sp_pred} r{residual_fp32}")


@pytest.mark.parametrize("L", [64, 200])
def test_short_rows_and_batch_of_one(L):
    cfg = _electra(128, 2, 512)
    sd = _random_state_dict(cfg, "electra", True, seed=5)
    for lens in ([L], [L, L // 2, 3]):
        batch = _batch(cfg, lens, L, 4, seed=L)
        ref = _reference(cfg, "electra", sd, batch, True)
        m = _model(cfg, "electra", sd, True)
        for mal in (0, 1, 35, L):
            _check(m, ref, batch, TOL_TINY, f"L={L} B={len(lens)} mal={mal}", max_ans_len=mal)


def test_bert_family_reader_matches_fp64_reference():
    cfg = transformers.BertConfig(vocab_size=1000, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=1024,
                                  max_position_embeddings=512, type_vocab_size=2, attn_implementation="eager")
    sd = _random_state_dict(cfg, "bert", True, seed=6)
    batch = _batch(cfg, [300, 40, 128], 300, 6, seed=7)
    _check(_model(cfg, "bert", sd, True), _reference(cfg, "bert", sd, batch, True), batch, TOL_TINY, "bert")


@pytest.mark.parametrize("L", [384, 512])
def test_electra_large_geometry_matches_fp64_reference(L):
    cfg = _electra(1024, 24, 4096, vocab=2000)
    sd = _random_state_dict(cfg, "electra", True, seed=8)
    batch = _batch(cfg, [L, L - 101, 57], L, 10, seed=9)
    ref = _reference(cfg, "electra", sd, batch, True)
    _check(_model(cfg, "electra", sd, True), ref, batch, TOL_LARGE, f"large L={L}", max_ans_len=35)


def test_token_type_ids_may_be_absent():
    """batch.get('token_type_ids', None) is None -> every token has type 0, as HF does."""
    cfg = _electra(128, 1, 512)
    sd = _random_state_dict(cfg, "electra", False, seed=10)
    batch = _batch(cfg, [90, 33], 90, 0, seed=11)
    ref_batch = dict(batch, token_type_ids=torch.zeros_like(batch["token_type_ids"]))
    ref = _reference(cfg, "electra", sd, ref_batch, False)
    nott = {k: v for k, v in batch.items() if k != "token_type_ids"}
    _check(_model(cfg, "electra", sd, False), ref, nott, TOL_TINY, "no token types")
