"""CPU: the host statements of the whole encoder's backward (tests/encoder_chain_ref.py) hold each other. model64 is the oracle's forward and
tests/mhop_loss_ref.py's loss; a second correct implementation of the device chain's numerics (regime_b: fp32 arithmetic, the batch reversed)
passes criterion E against the reference regime, and each wiring mutation fails it on at least one tensor. Every line prints its figures."""
import numpy as np
import pytest
import torch

import encoder_chain_ref as ch
import mhop_loss_ref
from oracle import roberta_torch

GEOM = ch.GEOM


@pytest.fixture(scope="module")
def sd():
    return ch.state_dict()


@pytest.fixture(scope="module")
def dense(sd):
    """the L = 48 batch under the fixed cotangent: model64 and the regime, computed once"""
    ids, mask = ch.batch("L48")
    G = ch.cotangent(len(ids))
    emb64, g64 = ch.grads_cotangent("model64", sd, GEOM, ids, mask, G)
    emb_reg, g_reg = ch.grads_cotangent("regime", sd, GEOM, ids, mask, G)
    return dict(ids=ids, mask=mask, G=G, emb64=emb64, g64=g64, emb_reg=emb_reg, g_reg=g_reg)


@pytest.fixture(scope="module")
def lossy(sd):
    """the in-batch loss over six encodes: model64 and the regime, computed once"""
    batches = ch.loss_batches()
    return dict(batches=batches, m64=ch.grads_loss("model64", sd, GEOM, batches), reg=ch.grads_loss("regime", sd, GEOM, batches))


def test_model64_forward_is_the_oracle(sd, dense):
    for name in ch.BATCHES:
        ids, mask = ch.batch(name)
        want = roberta_torch.encode(sd, GEOM, ids, mask, torch.float64).numpy()
        with torch.no_grad():
            got = ch.model64(ch.leaves(sd), GEOM, ids, mask).numpy()
        assert np.abs(got - want).max() <= 1e-9, name
    assert np.abs(dense["emb64"] - roberta_torch.encode(sd, GEOM, dense["ids"], dense["mask"], torch.float64).numpy()).max() <= 1e-9
    # the regime's forward is the oracle's restated mode-2 dataflow up to the roundings that regime keeps fp32 there (scores, P V, the GELU's
    # input) and the fp16 head: inside the encoder test's TINY bar against fp64
    err = np.abs(dense["emb_reg"] - dense["emb64"])
    print(f"regime forward against model64: max {err.max():.3e} mean {err.mean():.3e}")
    assert err.max() <= 6e-3 and err.mean() <= 1.2e-3


def test_model64_loss_gradients_are_mhop_loss_ref(lossy):
    loss, _, emb, demb = lossy["m64"]
    ref = mhop_loss_ref.loss_and_grads({k: emb[k] for k in ch.KEYS})
    assert abs(loss - ref["loss"]) <= 1e-9 * max(1.0, abs(ref["loss"]))
    for k in ch.KEYS:
        assert np.abs(demb[k] - ref["grads"][k]).max() <= 1e-12, k
    # and the regime's loss is that helper's mode O1 on the regime's embeddings
    loss, _, emb, demb = lossy["reg"]
    ref = mhop_loss_ref.loss_and_grads({k: emb[k] for k in ch.KEYS}, o1=True)
    assert abs(loss - ref["loss"]) <= 1e-9 * max(1.0, abs(ref["loss"]))
    for k in ch.KEYS:
        assert np.abs(demb[k] - ref["grads"][k]).max() <= 1e-12, k


def test_key_bias_gradient_is_zero_and_unused_rows_are_exact_zeros(dense, lossy):
    """softmax is shift-invariant along the keys: in fp64 the key bias's gradient is rounding noise next to its neighbours'"""
    for g64, batches in ((dense["g64"], [(dense["ids"], dense["mask"])]), (lossy["m64"][1], list(lossy["batches"].values()))):
        for k in ch.zero_grad_names():
            mine, qb = np.abs(g64[k]).max(), np.abs(g64[k.replace("key", "query")]).max()
            print(f"{k}: max |g64| {mine:.3e}, the query bias's {qb:.3e}")
            assert mine <= 1e-12 * qb
        zr = ch.zero_rows(batches)
        assert zr.any() and not zr.all()
        assert not g64["encoder.embeddings.word_embeddings.weight"][zr].any()
        assert np.abs(g64["encoder.embeddings.word_embeddings.weight"][~zr]).max(axis=1).min() > 0


@pytest.mark.parametrize("scale", [2.0 ** -10, 1.0, 256.0])
def test_regime_b_passes_criterion_e(sd, dense, scale):
    _, g_reg = ch.grads_cotangent("regime", sd, GEOM, dense["ids"], dense["mask"], dense["G"], scale) if scale != 1.0 else (None, dense["g_reg"])
    _, g_b = ch.grads_cotangent("regime_b", sd, GEOM, dense["ids"], dense["mask"], dense["G"], scale)
    rows, e_pool = ch.criterion_e(g_b, g_reg, dense["g64"])
    print(ch.table(rows, e_pool, f"regime_b, L48, scale {scale:g}"))
    print(f"worst share of the bar {max(r[4] for r in rows):.3f}")
    assert not ch.failures(rows)
    zr = ch.zero_rows([(dense["ids"], dense["mask"])])
    for g in (g_reg, g_b):
        assert not g["encoder.embeddings.word_embeddings.weight"][zr].any()


def test_regime_b_passes_criterion_e_under_the_loss(sd, lossy):
    g_b = ch.grads_loss("regime_b", sd, GEOM, lossy["batches"])[1]
    rows, e_pool = ch.criterion_e(g_b, lossy["reg"][1], lossy["m64"][1])
    print(ch.table(rows, e_pool, "regime_b, in-batch loss"))
    print(f"worst share of the bar {max(r[4] for r in rows):.3f}")
    assert not ch.failures(rows)


@pytest.mark.parametrize("mutation", ch.MUTATIONS)
def test_every_mutation_fails_criterion_e(sd, dense, lossy, mutation):
    if mutation == "last_call_only":  # only the loss uses the weights more than once
        g_m = ch.grads_loss("regime", sd, GEOM, lossy["batches"], mutation)[1]
        rows, _ = ch.criterion_e(g_m, lossy["reg"][1], lossy["m64"][1])
    else:
        _, g_m = ch.grads_cotangent("regime", sd, GEOM, dense["ids"], dense["mask"], dense["G"], 1.0, mutation)
        rows, _ = ch.criterion_e(g_m, dense["g_reg"], dense["g64"])
    bad = ch.failures(rows)
    print(f"{mutation}: {len(bad)} of {len(rows)} tensors over the bar, up to {max(r[4] for r in rows):.3g} x")
    assert bad
