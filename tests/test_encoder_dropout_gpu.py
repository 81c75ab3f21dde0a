"""GPU (-m gpu): the training-mode forward of the inference encoder (include/mdr_encoder_dropout.h, bound in
multihop_dense_retrieval_amd/momentum.py).

Kernel level: the fused LayerNorm equals dropout.packed_dropout followed by layernorm.packed_layer_norm, and the fused embedding equals
embedding.packed_embedding_layer_norm followed by dropout.packed_dropout(also16=True), bit for bit in both outputs, over both
lane-ownership paths (H % 256 == 0 with one, three and four float4 per lane; the generic path), one row, a few rows and more than one
block of rows, with the rows behind the valid count unwritten; a NaN and an Inf at positions the mask drops come out as NaN rows.
Whole forward: mdr_encoder_forward_dropout equals TrainableRetriever.encode(..., dropout=(seed, encode)) under no_grad bit for bit on TINY
and DEEP; both thresholds 0 is mdr_encoder_forward; one seed gives one result, another seed or encode another. The other residual modes
and a batch above MAX_TOKENS_PER_CALL are refused with messages."""
import numpy as np
import pytest
import torch

import encoder_chain_ref as ch
from encoder_chain_dev import same_bits
from guarded import SENTINEL, Guarded
from oracle import seeded

pytestmark = pytest.mark.gpu

CAP = 264                       # row capacity of every kernel-level case: 66 blocks of four rows
ROWS = (1, 5, 259)              # valid rows: one, a few inside one block and one more, more than one block with a ragged end
HIDDEN = (64, 128, 192, 256, 768, 1024)  # generic path (n = 1, 2, 3) and the H % 256 == 0 path (n4 = 1, 3, 4)
THRESHOLDS = (1, 26, 128, 255)
EPS = 1e-5
SEED = 0x9E3779B97F4A7C15
GEOMS = [pytest.param(seeded.TINY, id="TINY"), pytest.param(seeded.DEEP, id="DEEP")]


def f32(name, shape, std=1.0, mean=0.0):
    return torch.from_numpy(seeded.normal(77, name, shape, std, mean).astype(np.float32)).cuda()


def rows_tensor(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


@pytest.fixture(scope="module")
def ln_inputs():
    """per H: (x16, res32, weight, bias), drawn once and left unchanged"""
    return {H: (f32(f"x.{H}", (CAP, H), 2.0).half(), f32(f"res.{H}", (CAP, H)), f32(f"g.{H}", (H,), 0.1, 1.0), f32(f"b.{H}", (H,), 0.1)) for H in HIDDEN}


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("H", HIDDEN)
def test_fused_layernorm_is_dropout_then_layernorm(ln_inputs, H, rows):
    from multihop_dense_retrieval_amd import dropout, momentum
    from multihop_dense_retrieval_amd.layernorm import packed_layer_norm
    x16, res32, g, b = ln_inputs[H]
    n = rows_tensor(rows)
    for T in THRESHOLDS:
        site = dropout.site_of(T % 6, T % 64, "ao")
        assert dropout.threshold(T / 256.0) == T
        want16, want32 = packed_layer_norm(dropout.packed_dropout(x16, T / 256.0, SEED, site, n), res32, g, b, EPS, n, True)
        o16, o32 = Guarded(CAP, (H,), torch.float16, 2, 2, name="y16"), Guarded(CAP, (H,), torch.float32, 2, 2, name="y32")
        momentum.layer_norm_dropout(x16, res32, g, b, EPS, T, SEED, site, n, o16.own, o32.own)
        torch.cuda.synchronize()
        got16, got32 = o16.checked(o16.buf, valid=rows), o32.checked(o32.buf, valid=rows)
        assert same_bits(got16[:rows], want16[:rows]), (H, rows, T, "y16")
        assert same_bits(got32[:rows], want32[:rows]), (H, rows, T, "y32")
        if T == 128:  # the mask is live: the plain LayerNorm of the same rows gives other bits
            plain = packed_layer_norm(x16, res32, g, b, EPS, n, True)[1]
            assert not same_bits(plain[:rows], want32[:rows])
    # without a residual, and in place over the residual as the encoder calls it (out32 aliases res32)
    site = dropout.site_of(1, 2, "ff2")
    want16, want32 = packed_layer_norm(dropout.packed_dropout(x16, 0.1, SEED, site, n), None, g, b, EPS, n, True)
    got16, got32 = momentum.layer_norm_dropout(x16, None, g, b, EPS, 26, SEED, site, n)
    assert same_bits(got16, want16) and same_bits(got32, want32), (H, rows, "no residual")
    want16, want32 = packed_layer_norm(dropout.packed_dropout(x16, 0.1, SEED, site, n), res32, g, b, EPS, n, True)
    alias = res32.clone()
    got16, got32 = momentum.layer_norm_dropout(x16, alias, g, b, EPS, 26, SEED, site, n, None, alias)
    assert got32 is alias and same_bits(got16, want16) and same_bits(alias[:rows], want32[:rows]) and same_bits(alias[rows:], res32[rows:]), (H, rows, "in place")


@pytest.mark.parametrize("H", [192, 768])
def test_a_non_finite_value_at_a_dropped_position_is_nan(ln_inputs, H):
    """the factor is a multiplication, not a select: 0 * NaN and 0 * Inf are NaN, and a NaN in a row makes the row's LayerNorm NaN"""
    from multihop_dense_retrieval_amd import dropout, momentum
    x16, res32, g, b = ln_inputs[H]
    T, site, rows = 128, dropout.site_of(3, 1, "ao"), 5
    kept = dropout.dropout_rows(torch.ones((CAP, H), dtype=torch.float16, device="cuda"), T, SEED, site) != 0
    x = x16.clone()
    for row, value in ((1, float("nan")), (3, float("inf"))):
        col = int((~kept[row]).nonzero()[0])
        x[row, col] = value
    got16, got32 = momentum.layer_norm_dropout(x, res32, g, b, EPS, T, SEED, site, rows_tensor(rows))
    clean16, clean32 = momentum.layer_norm_dropout(x16, res32, g, b, EPS, T, SEED, site, rows_tensor(rows))
    for row in range(rows):
        if row in (1, 3):
            assert bool(torch.isnan(got16[row]).all()) and bool(torch.isnan(got32[row]).all()), (H, row)
        else:
            assert same_bits(got16[row], clean16[row]) and same_bits(got32[row], clean32[row]), (H, row)


def packed(ids, mask, pad_id):
    from multihop_dense_retrieval_amd import _lib
    from multihop_dense_retrieval_amd._lib import ptr
    B, L = ids.shape
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device="cuda")  # noqa: E731
    lens, cu, total, order, src, pid = i32(B), i32(B + 1), i32(1), i32(B), i32(B * L), i32(B * L)
    _lib.call(_lib.lib().mdr_test_pack, ptr(ids), ptr(mask), B, L, pad_id, ptr(lens), ptr(cu), ptr(total), ptr(order), ptr(src), ptr(pid), dev=ids.device)
    return total, src, pid


EMB_LENS = {1: (0, 0, 1, 0, 0, 0, 0, 0), 5: (2, 0, 3, 0, 0, 0, 0, 0), 259: (33, 33, 33, 28, 33, 33, 33, 33)}  # B = 8, L = 33: cap 264


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("H", HIDDEN)
def test_fused_embedding_is_embedding_then_dropout(H, rows):
    from multihop_dense_retrieval_amd import dropout, momentum
    from multihop_dense_retrieval_amd.embedding import packed_embedding_layer_norm
    B, L, vocab, max_pos, pad_id = 8, 33, 97, 40, 1
    lens = EMB_LENS[rows]
    assert sum(lens) == rows and B * L == CAP
    ids = torch.from_numpy(seeded.integers(5, f"emb.ids.{rows}", (B, L), 3, vocab).astype(np.int64)).cuda()
    mask = torch.zeros((B, L), dtype=torch.int64, device="cuda")
    for i, n in enumerate(lens):
        mask[i, :n] = 1
    ids[mask == 0] = pad_id
    total, src, pid = packed(ids, mask, pad_id)
    word, pos, type0 = f32(f"word.{H}", (vocab, H), 0.5), f32(f"pos.{H}", (max_pos, H), 0.5), f32(f"type.{H}", (H,), 0.5)
    g, b = f32(f"eg.{H}", (H,), 0.1, 1.0), f32(f"eb.{H}", (H,), 0.1)
    h16, h32 = packed_embedding_layer_norm(ids, src, pid, total, word, pos, type0, g, b, EPS, CAP, pad_id, True)
    for T in THRESHOLDS:
        site = dropout.site_of(T % 6, 0, "emb")
        want32, want16 = dropout.packed_dropout(h32, T / 256.0, SEED, site, total, True)
        o16, o32 = Guarded(CAP, (H,), torch.float16, 2, 2, name="y16"), Guarded(CAP, (H,), torch.float32, 2, 2, name="y32")
        momentum.embedding_layer_norm_dropout(ids, src, pid, total, word, pos, type0, g, b, EPS, CAP, T, SEED, site, o16.own, o32.own)
        torch.cuda.synchronize()
        got16, got32 = o16.checked(o16.buf, valid=rows), o32.checked(o32.buf, valid=rows)
        assert same_bits(got16[:rows], want16[:rows]), (H, rows, T, "y16")
        assert same_bits(got32[:rows], want32[:rows]), (H, rows, T, "y32")
        if T == 128:
            assert not same_bits(h32[:rows], want32[:rows])


# ---- the whole forward ------------------------------------------------------------------------------------------------------------------------
LENS = (40, 1, 17, 33, 8)  # B = 5, L = 40: ragged, the shortest and the longest a row can be
ENCODES = (2, 5)
RATES = ((0.1, 0.1), (0.5, 0.0), (0.0, 0.3))


def config_of(geom, p_hidden=0.0, p_attn=0.0):
    from multihop_dense_retrieval_amd import retriever
    cfg = retriever.RobertaConfig(vocab_size=geom["vocab"], hidden_size=geom["hidden"], num_hidden_layers=geom["layers"], num_attention_heads=geom["heads"],
                                  intermediate_size=geom["ffn"], max_position_embeddings=geom["max_pos"], layer_norm_eps=geom["ln_eps"], pad_token_id=geom["pad_id"])
    cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = p_hidden, p_attn
    return cfg


def trainable(geom, p_hidden, p_attn):
    from multihop_dense_retrieval_amd import train
    sd = seeded.make_state_dict(ch.WEIGHT_SEED, geom)
    m = train.TrainableRetriever(config_of(geom, p_hidden, p_attn), None)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.cuda().train()


@pytest.mark.parametrize("geom", GEOMS)
def test_forward_dropout_is_the_training_chains(geom):
    from multihop_dense_retrieval_amd import dropout, momentum
    ids, mask = (torch.from_numpy(a).cuda() for a in ch.make_batch(40, LENS, 53, geom))
    plain = None
    for p_hidden, p_attn in RATES:
        model = trainable(geom, p_hidden, p_attn)
        served = model.inference()
        T_hid, T_att = dropout.threshold(p_hidden), dropout.threshold(p_attn)
        if plain is None:
            plain = served.encode_seq(ids, mask).clone()
            assert same_bits(momentum.encode_dropout(served, ids, mask, 0, 0, SEED, 2), plain), "both thresholds 0 is not mdr_encoder_forward"
        outs = {}
        for encode in ENCODES:
            with torch.no_grad():
                want = model.encode(ids, mask, None, (SEED, encode))
            got = momentum.encode_dropout(served, ids, mask, T_hid, T_att, SEED, encode)
            assert bool(torch.isfinite(got).all())
            assert same_bits(got, want), (p_hidden, p_attn, encode, float((got - want).abs().max()))
            assert same_bits(momentum.encode_dropout(served, ids, mask, T_hid, T_att, SEED, encode), got), "two calls with one seed differ"
            assert not same_bits(got, plain), "the mask changed nothing: this test shows nothing"
            outs[encode] = got
        assert not same_bits(outs[2], outs[5]), "another encode gave the same bits"
        assert not same_bits(momentum.encode_dropout(served, ids, mask, T_hid, T_att, SEED + 1, 2), outs[2]), "another seed gave the same bits"
        assert same_bits(served.encode_seq(ids, mask), plain), "the training-mode forward changed the inference forward"


def test_other_residual_modes_and_an_over_long_batch_are_refused(monkeypatch):
    import ctypes
    from multihop_dense_retrieval_amd import _lib, momentum, retriever
    from multihop_dense_retrieval_amd._lib import ptr
    geom = seeded.TINY
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in seeded.make_state_dict(ch.WEIGHT_SEED, geom).items()}
    ids, mask = (torch.from_numpy(a).cuda() for a in ch.make_batch(40, LENS, 53, geom))
    for mode in (0, 1):
        monkeypatch.setenv("MDR_RESIDUAL_FP32", str(mode))
        enc = retriever.RobertaRetriever(config_of(geom), None)
        monkeypatch.delenv("MDR_RESIDUAL_FP32")
        enc.load_state_dict(sd)
        enc.to("cuda")
        with pytest.raises(NotImplementedError, match="residual_fp32 = 2"):
            momentum.encode_dropout(enc, ids, mask, 26, 26, SEED, 2)
        need = int(_lib.lib().mdr_encoder_workspace_bytes(enc._h, 5, 40))
        ws, out = torch.empty(need, dtype=torch.uint8, device="cuda"), torch.full((5, geom["hidden"]), SENTINEL, device="cuda")
        rc = momentum.lib().mdr_encoder_forward_dropout(enc._h, ptr(ids), ptr(mask), 5, 40, 26, 26, SEED, 2, ptr(out), ptr(ws), need, _lib.current_stream_ptr())
        assert rc == -1 and b"residual_fp32 = 2" in _lib.lib().mdr_last_error(), (rc, _lib.lib().mdr_last_error())
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), "a refused call wrote its output"
    enc = retriever.RobertaRetriever(config_of(geom), None)
    enc.load_state_dict(sd)
    enc.to("cuda")
    enc.MAX_TOKENS_PER_CALL = 5 * 40 - 1
    with pytest.raises(ValueError, match="MAX_TOKENS_PER_CALL"):
        momentum.encode_dropout(enc, ids, mask, 26, 26, SEED, 2)
    for bad in (dict(T_hidden=256), dict(T_attention=-1), dict(encode=6)):
        kw = dict(T_hidden=26, T_attention=26, seed=SEED, encode=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            momentum.encode_dropout(enc, ids, mask, **kw)
    assert enc.graph_captures == 0 and enc.graph_replays == 0
