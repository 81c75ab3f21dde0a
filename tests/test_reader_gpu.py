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
from oracle import fp  # noqa: E402

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


def _reference_fn(config, family, sd, sp_pred):
    """qa_model.py QAModel.forward in fp64 on the device: HF ElectraModel / BertModel (transformers, eager attention) + the heads.
    Returns fn(batch) -> outputs, so that one fp64 model serves several batches (or several row chunks of one)."""
    cls = transformers.ElectraModel if family == "electra" else transformers.BertModel
    kw = {} if family == "electra" else {"add_pooling_layer": True}
    enc = cls(config, **kw).to(DEV).double().eval()
    missing, unexpected = enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}, strict=False)
    assert not [m for m in missing if "position_ids" not in m] and not unexpected, (missing, unexpected)
    W = {k: v.to(DEV).double() for k, v in sd.items() if not k.startswith("encoder.") or "pooler" in k}

    def fn(batch):
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
    return fn


def _rows(batch, lo, hi):
    return {k: v[lo:hi] for k, v in batch.items()}


def _reference(config, family, sd, batch, sp_pred, rows=None, fn=None):
    """The fp64 reference of one batch; with `rows`, computed that many rows at a time (rows are independent in the reference, and the
    [B, heads, L, L] fp64 scores of a large batch need not exist at once)."""
    fn = fn or _reference_fn(config, family, sd, sp_pred)
    B = batch["input_ids"].shape[0]
    if rows is None or B <= rows:
        return fn(batch)
    parts = [fn(_rows(batch, i, i + rows)) for i in range(0, B, rows)]
    return {k: None if parts[0][k] is None else torch.cat([p[k] for p in parts]) for k in parts[0]}


def _model(config, family, sd, sp_pred):
    name = "google/electra-test-discriminator" if family == "electra" else "bert-test-uncased"
    m = reader.QAModel(config, types.SimpleNamespace(model_name=name, sp_pred=sp_pred))
    m.load_state_dict(sd)
    return m.to(DEV).eval()


def _errors(out, ref):
    """max |err| / mean |reference output| per output, the unit of the bars below (the logits over the unmasked positions)."""
    finite = torch.isfinite(ref["start_logits"])
    scale = ref["start_logits"][finite].abs().mean().item()
    errs = {k: (out[k].double() - ref[k])[finite].abs().max().item() / scale for k in ("start_logits", "end_logits")}
    errs["rank"] = (out["rank_score"].double() - ref["rank_score"]).abs().max().item() / max(ref["rank_score"].abs().mean().item(), 1e-3)
    if ref["sp_score"] is not None:
        errs["sp"] = (out["sp_score"].double() - ref["sp_score"]).abs().max().item() / max(ref["sp_score"].abs().mean().item(), 1e-3)
    return errs


def _check(m, ref, batch, tol, label, max_ans_len=30):
    out = m(batch)
    dec = m.decode(batch, max_ans_len, with_logits=True)
    for k in ("start_logits", "end_logits"):
        got, want = out[k], ref[k]
        assert got.dtype == torch.float16
        assert torch.equal(torch.isinf(got), torch.isinf(want)), k  # -inf exactly where the reference masks
        assert torch.equal(dec[k].view(torch.int16), got.view(torch.int16)), k  # the fused path computes the same logits
    assert out["rank_score"].shape == ref["rank_score"].shape
    errs = _errors(out, ref)
    if ref["sp_score"] is not None:
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


# ---- promises of include/mdr_reader.h at the edges of its inputs --------------------------------------------------------------------------------------
def test_sp_offsets_outside_the_row_and_at_zero():
    """An sp offset at or past the row's length (inside the padding, at L, far past L) or negative: sp_score -inf, sp_prob 0. Offset 0 on a real row:
    sp_score is the finite sp logit of position 0 and sp_prob is 0 (predict()'s sent_offsets == 0 mask)."""
    cfg = _electra(128, 1, 512)
    sd = _random_state_dict(cfg, "electra", True, seed=20)
    L = 50
    batch = _batch(cfg, [50, 20, 33], L, 6, seed=21)
    so = torch.tensor([[10, 0, 49, 50, -1, 12], [20, 5, 30, 49, 19, 0], [0, 33, 10 ** 9, -(10 ** 9), 32, -5]])
    valid = torch.tensor([[1, 1, 1, 0, 0, 1], [0, 1, 0, 0, 1, 1], [1, 0, 0, 0, 1, 0]], dtype=torch.bool)
    ref = _reference(cfg, "electra", sd, dict(batch, sent_offsets=torch.where(valid, so, torch.zeros_like(so))), True)
    m = _model(cfg, "electra", sd, True)
    dec = m.decode(dict(batch, sent_offsets=so), 30, with_logits=True)
    got, prob, v = dec["sp_score"].cpu(), dec["sp_prob"].cpu(), valid
    assert bool((got[~v] == -float("inf")).all()) and bool((prob[~v] == 0).all())
    assert bool(torch.isfinite(got[v]).all())
    want = ref["sp_score"].cpu()
    assert (got[v].double() - want[v]).abs().max().item() <= TOL_TINY * want[v].abs().mean().item()
    assert bool((prob[so == 0] == 0).all()) and bool((prob[v & (so != 0)] > 0).all())
    assert torch.equal(prob.view(torch.int16), got.float().masked_fill(so.eq(0), -float("inf")).half().sigmoid().view(torch.int16))


def test_paragraph_mask_on_padding_and_values_other_than_0_and_1():
    """paragraph_mask = 1 on padded positions, and values 2 and -1: the logits there are -inf (only == 1 on a real token keeps a position); a row whose
    whole band is masked that way decodes to (0, 0) with a span score of -inf."""
    cfg = _electra(128, 2, 512)
    sd = _random_state_dict(cfg, "electra", True, seed=22)
    L = 64
    clean = _batch(cfg, [64, 30, 41, 9], L, 4, seed=23)
    pm = clean["paragraph_mask"].clone()
    pm[1, 30:] = 1   # on the padding
    pm[0, 20:25] = 2
    pm[0, 40] = -1
    pm[2][pm[2] == 1] = 2  # the whole band of row 2
    pm[3, 9:] = 1
    want_pm = torch.where((pm == 1) & (clean["attention_mask"] == 1), 1, 0)
    assert int(want_pm[2].sum()) == 0 and int(want_pm[0].sum()) == int(clean["paragraph_mask"][0].sum()) - 6
    ref = _reference(cfg, "electra", sd, dict(clean, paragraph_mask=want_pm), True)
    m = _model(cfg, "electra", sd, True)
    dirty = dict(clean, paragraph_mask=pm)
    _check(m, ref, dirty, TOL_TINY, "paragraph_mask edges")  # the -inf pattern is the reference's, exactly
    dec = m.decode(dirty, 30)
    assert (int(dec["start"][2]), int(dec["end"][2])) == (0, 0) and float(dec["span_score"][2]) == -float("inf")
    assert bool(torch.isfinite(dec["span_score"][[0, 1, 3]].float()).all())


def test_no_sentences_and_extreme_max_ans_len():
    """n_sent = 0: sp_pred without sent_offsets gives no sp outputs and leaves the others alone; max_ans_len = 0 and >= L through decode()."""
    cfg = _electra(128, 1, 512)
    sd = _random_state_dict(cfg, "electra", True, seed=24)
    L = 70
    batch = _batch(cfg, [70, 12, 45], L, 3, seed=25)
    m = _model(cfg, "electra", sd, True)
    nosent = {k: v for k, v in batch.items() if k != "sent_offsets"}
    ref = _reference(cfg, "electra", sd, batch, True)
    out, full = m(nosent), m(batch)
    assert out["sp_score"] is None
    for k in ("start_logits", "end_logits", "rank_score"):
        assert torch.equal(out[k].view(torch.int16), full[k].view(torch.int16)), k
    for mal in (0, L - 1, L, L + 1000):
        dec = m.decode(nosent, mal, with_logits=True)
        assert dec["sp_prob"] is None and dec["sp_score"] is None
        s, e, sc = reader.span_search_reference(out["start_logits"], out["end_logits"], mal)
        assert torch.equal(dec["start"], s) and torch.equal(dec["end"], e) and torch.equal(dec["span_score"].view(torch.int16), sc.view(torch.int16)), mal
        if mal == 0:
            assert torch.equal(dec["start"], dec["end"])
        _check(m, ref, batch, TOL_TINY, f"max_ans_len={mal}", max_ans_len=mal)


def test_bad_inputs_are_refused_on_the_host():
    """Errors instead of launches: L = 513, L > max_position_embeddings, a left-padded mask, embeddings_project (ELECTRA-small) by config and by tensor name
    through the C ABI, sp outputs from a reader created with has_sp = 0. Every one of these is decided before any kernel is launched."""
    import ctypes
    from multihop_dense_retrieval_amd import _lib
    cfg = _electra(128, 1, 512)
    sd = _random_state_dict(cfg, "electra", False, seed=26)
    m = _model(cfg, "electra", sd, False)

    def rows(B, L):
        return {"input_ids": torch.ones((B, L), dtype=torch.int64), "attention_mask": torch.ones((B, L), dtype=torch.int64),
                "token_type_ids": torch.zeros((B, L), dtype=torch.int64), "paragraph_mask": torch.ones((B, L), dtype=torch.int64)}
    with pytest.raises(ValueError, match="513"):
        m(rows(2, 513))
    left = rows(2, 16)
    left["attention_mask"][1, :5] = 0
    with pytest.raises(ValueError, match="right-padded"):
        m(left)
    hole = rows(2, 16)
    hole["attention_mask"][0, 7] = 0
    with pytest.raises(ValueError, match="right-padded"):
        m(hole)
    # 128 positions: L = 128 runs, L = 129 is refused by the library (seq_len <= max_pos)
    short = transformers.ElectraConfig(vocab_size=1000, hidden_size=128, embedding_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=512,
                                       max_position_embeddings=128, type_vocab_size=2, layer_norm_eps=1e-12, attn_implementation="eager")
    ms = _model(short, "electra", _random_state_dict(short, "electra", False, seed=27), False)
    assert bool(torch.isfinite(ms(rows(2, 128))["rank_score"].float()).all())
    with pytest.raises(_lib.MdrError, match="max_pos"):
        ms(rows(2, 129))
    # ELECTRA-small: refused by the Python class from the config, and by mdr_reader_create from the tensor name
    small = transformers.ElectraConfig(vocab_size=1000, hidden_size=256, embedding_size=128, num_hidden_layers=1, num_attention_heads=4, intermediate_size=512)
    with pytest.raises(NotImplementedError, match="embeddings_project"):
        reader.QAModel(small, types.SimpleNamespace(model_name="google/electra-small-discriminator", sp_pred=False))
    keep = {k: v.float().contiguous() for k, v in sd.items()}
    keep["encoder.embeddings_project.weight"] = torch.zeros((128, 128))
    arr = (_lib.Tensor * len(keep))(*[_lib.Tensor(k.encode(), ctypes.c_void_p(v.data_ptr()), v.numel()) for k, v in keep.items()])
    rc_cfg = reader.ReaderConfig(cfg.vocab_size, 128, 1, 2, 512, 512, 2, 1e-12, 2, 0, reader.POOLER_HEAD)
    h = ctypes.c_void_p()
    rc = reader.lib().mdr_reader_create(ctypes.byref(rc_cfg), arr, len(keep), 0, 0, None, ctypes.byref(h))
    assert rc != 0 and not h.value and b"embeddings_project" in reader.lib().mdr_last_error()
    # has_sp = 0 and sp outputs asked for through the C ABI
    B, L, NS = 2, 16, 3
    b = {k: v.to(DEV) for k, v in rows(B, L).items()}
    so = torch.ones((B, NS), dtype=torch.int64, device=DEV)
    f16 = dict(dtype=torch.float16, device=DEV)
    bufs = [torch.zeros((B, L), **f16), torch.zeros((B, L), **f16), torch.zeros((B, 1), **f16), torch.zeros((B, NS), **f16), torch.zeros((B, NS), **f16)]
    ws = torch.empty(int(reader.lib().mdr_reader_workspace_bytes(m._h, B, L, NS)), dtype=torch.uint8, device=DEV)
    for sp_score, sp_prob in ((bufs[3], None), (None, bufs[4])):
        o = reader.ReaderOutputs(reader._ptr(bufs[0]), reader._ptr(bufs[1]), reader._ptr(bufs[2]), reader._ptr(sp_score), reader._ptr(sp_prob), None, None, None)
        rc = reader.lib().mdr_reader_forward(m._h, reader._ptr(b["input_ids"]), reader._ptr(b["attention_mask"]), reader._ptr(b["token_type_ids"]),
                                             reader._ptr(b["paragraph_mask"]), reader._ptr(so), B, L, NS, -1, ctypes.byref(o), reader._ptr(ws), ws.numel(),
                                             _lib.current_stream_ptr(torch.device(DEV, 0)))
        assert rc != 0 and b"has_sp" in reader.lib().mdr_last_error()
    torch.cuda.synchronize()
    assert all(float(t.abs().sum()) == 0 for t in bufs)  # nothing ran


# ---- the heads' rounding points, exactly --------------------------------------------------------------------------------------------------------------
def _ulp16(v):
    """Spacing of fp16 at |v| (fp64 tensor): 2^(floor(log2 |v|) - 10), 2^-24 below the smallest normal."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14))).clamp_min(-14.0)
    return torch.exp2(e - 10.0)


@pytest.mark.parametrize("hidden", [128, 768, 1024])
def test_head_rounding_points(hidden):
    """csrc/mdr_reader.inl lists the heads' rounding points (apex O1): fp16 input, fp16 weight and fp16 bias, fp32 accumulation, ONE rounding to fp16. The fp64
    comparison above has bars sized for the trunk's noise (1.5e-2 of the mean logit), which would hide a second rounding or a bias at the wrong precision.
    Here the LAST output.LayerNorm gets weight 0, so every final hidden state is that LayerNorm's bias beta exactly, whatever the trunk did, and the input of
    the heads is fp16(beta), known on the host. (All tokens carry the same state: this says nothing about indexing, which the other tests cover.)

    start / end / sp. Exact value r = sum_i fp16(beta_i) fp16(w_i) + fp16(b), in fp64 (the products are exact there). The kernel computes fl32(r) with an
    accumulation error of at most H 2^-24 sum_i |beta_i w_i| (the standard n u sum|x_i y_i| bound with u = 2^-24; the kernel's longest chain is H / 64 + 6 adds
    and the bias add, so H covers it) and rounds once: |got - r| <= ulp16 / 2 + H 2^-24 sum_i |beta_i w_i|, the spacing taken at max(|got|, |r|). A dot rounded
    to fp16 before the bias is added errs by up to one ulp16. Each model gives only three such values, hence the seeds.

    rank. d_j = fp16(sum_i fp16(beta_i) fp16(Wp_ji) + fp16(bp_j)), t_j = fp16(tanh(d_j)), r = sum_j t_j fp16(w_j) + fp16(b). The pooler dense is a GEMM whose
    fp32 sum and bias may land on the other side of a rounding boundary: one ulp16(d_j) of slack per dense output. tanh is monotone with slope sech^2 <= 1,
    largest over [|d_j| - ulp, |d_j| + ulp] at the smaller end, so the kernel's tanh argument moves tanh by at most ulp16(d_j) sech^2(max(|d_j| - ulp16(d_j), 0));
    its fp16 rounding (and tanhf's last bits) can add one more spacing of t_j: |t'_j - t_j| <= tau_j = ulp16(d_j) sech^2(...) + ulp16(t_j). Through the dot:
    |got - r| <= ulp16 / 2 + H 2^-24 sum_j (|t_j| + tau_j) |w_j| + sum_j tau_j |w_j|."""
    worst = {"start": 0.0, "end": 0.0, "sp": 0.0, "rank": 0.0}
    for seed in range(12):
        cfg = _electra(hidden, 1, 256)
        sd = _random_state_dict(cfg, "electra", True, seed=100 + seed)
        g = torch.Generator().manual_seed(200 + seed)
        sd["encoder.encoder.layer.0.output.LayerNorm.weight"] = torch.zeros(hidden)
        sd["encoder.encoder.layer.0.output.LayerNorm.bias"] = torch.randn(hidden, generator=g)
        batch = _batch(cfg, [40, 17, 1], 40, 4, seed=seed)
        m = _model(cfg, "electra", sd, True)
        dec = m.decode(batch, 30, with_logits=True)
        x = sd["encoder.encoder.layer.0.output.LayerNorm.bias"].half().double()

        def h16(name):
            return sd[name].half().double()

        def dot_check(got, w, b, terms, extra, label):
            r = (terms * w).sum() + b
            got = got.double().flatten()
            bound = 0.5 * _ulp16(torch.maximum(got.abs(), r.abs())) + hidden * fp.U32 * ((terms.abs() + extra) * w.abs()).sum() + (extra * w.abs()).sum()
            err = (got - r).abs()
            worst[label] = max(worst[label], (err / bound).max().item())
            assert bool((err <= bound).all()), f"hidden {hidden} seed {seed} {label}: got {got[err.argmax()].item()!r} exact {r.item()!r} |err| {err.max().item():.3e} bound {bound.min().item():.3e}"

        zero = torch.zeros(hidden, dtype=torch.float64)
        wqa, bqa = h16("qa_outputs.weight"), h16("qa_outputs.bias")
        for i, k in enumerate(("start", "end")):
            lg = dec[k + "_logits"].cpu()
            finite = torch.isfinite(lg)
            assert torch.equal(finite, batch["paragraph_mask"].eq(1)) and int(finite.sum()) > 20
            dot_check(lg[finite], wqa[i], bqa[i], x, zero, k)
        dot_check(dec["sp_score"].cpu(), h16("sp.weight")[0], h16("sp.bias")[0], x, zero, "sp")
        d = (h16("pooler.dense.weight") @ x + h16("pooler.dense.bias")).half().double()
        t = torch.tanh(d).half().double()
        ud = _ulp16(d)
        tau = ud / torch.cosh((d.abs() - ud).clamp_min(0.0)) ** 2 + _ulp16(t)
        dot_check(dec["rank_score"].cpu(), h16("rank.weight")[0], h16("rank.bias")[0], t, tau, "rank")
        so = batch["sent_offsets"]
        want_prob = dec["sp_score"].cpu().float().masked_fill(so.eq(0), float("-inf")).half().sigmoid()
        assert torch.equal(dec["sp_prob"].cpu().view(torch.int16), want_prob.view(torch.int16))
    print(f"[reader heads hidden={hidden}] worst |err| / bound: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
