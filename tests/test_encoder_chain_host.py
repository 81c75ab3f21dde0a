"""CPU: the host statements of the whole encoder's backward (tests/encoder_chain_ref.py) hold each other, on both geometries of the chain tests:
oracle.seeded.TINY (two layers: the first and the CLS-only last) and DEEP (four layers: the smallest depth with a full layer behind a full
layer). model64 is the oracle's forward and tests/mhop_loss_ref.py's loss; a second correct implementation of the device chain's numerics
(regime_b: fp32 arithmetic, the batch reversed) passes criterion E against the reference regime, and each wiring mutation fails it on at least
one tensor. The mutations of a middle layer change NOTHING on TINY and fail on DEEP: that is why DEEP exists. Every line prints its figures.

The last part holds the same statements with dropout at every site (masks from the replica of tests/dropout_ref.py as constant factors): the site
function is injective, every mask of every device batch keeps and drops, the batches meet criterion E's premises under the masks, the masked regime
and regime_b pass criterion E against the masked fp64 model, each wiring defect of the dropout recipe fails it, and masks of all ones are no dropout.

A test that had no parameter keeps its name on TINY and has a sibling `..._on_deep`; a parametrised one keeps its TINY ids and gains `DEEP-...`."""
import functools

import numpy as np
import pytest
import torch

import encoder_chain_ref as ch
import mhop_loss_ref
from oracle import roberta_torch, seeded

GEOMS = {"TINY": seeded.TINY, "DEEP": seeded.DEEP}
TINY_MUTATIONS = tuple(m for m in ch.MUTATIONS if m not in ch.MID_MUTATIONS)


def both(values):
    """the parameters (geometry name, value): TINY's ids are the bare values, as before the second geometry came"""
    return [pytest.param(gn, v, id=(str(v) if gn == "TINY" else f"{gn}-{v}")) for gn in GEOMS for v in values]


@functools.lru_cache(maxsize=None)
def sd_of(gn):
    return ch.state_dict(GEOMS[gn])


@functools.lru_cache(maxsize=None)
def dense_of(gn):
    """the L = 48 batch under the fixed cotangent: model64 and the regime, computed once per geometry"""
    geom, sd = GEOMS[gn], sd_of(gn)
    ids, mask = ch.batch("L48", geom)
    G = ch.cotangent(len(ids), geom)
    emb64, g64 = ch.grads_cotangent("model64", sd, geom, ids, mask, G)
    emb_reg, g_reg = ch.grads_cotangent("regime", sd, geom, ids, mask, G)
    return dict(ids=ids, mask=mask, G=G, emb64=emb64, g64=g64, emb_reg=emb_reg, g_reg=g_reg)


@functools.lru_cache(maxsize=None)
def lossy_of(gn):
    """the in-batch loss over six encodes: model64 and the regime, computed once per geometry"""
    geom, sd = GEOMS[gn], sd_of(gn)
    batches = ch.loss_batches(geom)
    return dict(batches=batches, m64=ch.grads_loss("model64", sd, geom, batches), reg=ch.grads_loss("regime", sd, geom, batches))


def _model64_forward_is_the_oracle(gn):
    geom, sd, dense = GEOMS[gn], sd_of(gn), dense_of(gn)
    for name in ch.BATCHES:
        ids, mask = ch.batch(name, geom)
        want = roberta_torch.encode(sd, geom, ids, mask, torch.float64).numpy()
        with torch.no_grad():
            got = ch.model64(ch.leaves(sd), geom, ids, mask).numpy()
        assert np.abs(got - want).max() <= 1e-9, name
    assert np.abs(dense["emb64"] - roberta_torch.encode(sd, geom, dense["ids"], dense["mask"], torch.float64).numpy()).max() <= 1e-9
    # the regime's forward is the oracle's restated mode-2 dataflow up to the roundings that regime keeps fp32 there (scores, P V, the GELU's
    # input) and the fp16 head: on TINY inside the encoder test's TINY bar against fp64. That bar belongs to TINY; on DEEP the distance is
    # printed (it is the yardstick of the device forward there, tests/test_encoder_chain_gpu.py A)
    err = np.abs(dense["emb_reg"] - dense["emb64"])
    print(f"{gn}: regime forward against model64: max {err.max():.3e} mean {err.mean():.3e}")
    if gn == "TINY":
        assert err.max() <= 6e-3 and err.mean() <= 1.2e-3


def test_model64_forward_is_the_oracle():
    _model64_forward_is_the_oracle("TINY")


def test_model64_forward_is_the_oracle_on_deep():
    _model64_forward_is_the_oracle("DEEP")


def _model64_loss_gradients_are_mhop_loss_ref(gn):
    lossy = lossy_of(gn)
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


def test_model64_loss_gradients_are_mhop_loss_ref():
    _model64_loss_gradients_are_mhop_loss_ref("TINY")


def test_model64_loss_gradients_are_mhop_loss_ref_on_deep():
    _model64_loss_gradients_are_mhop_loss_ref("DEEP")


def _key_bias_gradient_is_zero_and_unused_rows_are_exact_zeros(gn):
    """softmax is shift-invariant along the keys: in fp64 the key bias's gradient is rounding noise next to its neighbours'"""
    geom, dense, lossy = GEOMS[gn], dense_of(gn), lossy_of(gn)
    assert len(ch.zero_grad_names(geom)) == geom["layers"]
    for g64, batches in ((dense["g64"], [(dense["ids"], dense["mask"])]), (lossy["m64"][1], list(lossy["batches"].values()))):
        for k in ch.zero_grad_names(geom):
            mine, qb = np.abs(g64[k]).max(), np.abs(g64[k.replace("key", "query")]).max()
            print(f"{gn}: {k}: max |g64| {mine:.3e}, the query bias's {qb:.3e}")
            assert mine <= 1e-12 * qb
        zr = ch.zero_rows(batches, geom)
        assert zr.any() and not zr.all()
        assert not g64["encoder.embeddings.word_embeddings.weight"][zr].any()
        assert np.abs(g64["encoder.embeddings.word_embeddings.weight"][~zr]).max(axis=1).min() > 0


def test_key_bias_gradient_is_zero_and_unused_rows_are_exact_zeros():
    _key_bias_gradient_is_zero_and_unused_rows_are_exact_zeros("TINY")


def test_key_bias_gradient_is_zero_and_unused_rows_are_exact_zeros_on_deep():
    _key_bias_gradient_is_zero_and_unused_rows_are_exact_zeros("DEEP")


@pytest.mark.parametrize("gn,scale", both([2.0 ** -10, 1.0, 256.0]))
def test_regime_b_passes_criterion_e(gn, scale):
    geom, sd, dense = GEOMS[gn], sd_of(gn), dense_of(gn)
    _, g_reg = ch.grads_cotangent("regime", sd, geom, dense["ids"], dense["mask"], dense["G"], scale) if scale != 1.0 else (None, dense["g_reg"])
    _, g_b = ch.grads_cotangent("regime_b", sd, geom, dense["ids"], dense["mask"], dense["G"], scale)
    rows, e_pool = ch.criterion_e(g_b, g_reg, dense["g64"], geom)
    assert len(rows) == len(ch.param_names(geom)) - geom["layers"]
    print(ch.table(rows, e_pool, f"{gn}: regime_b, L48, scale {scale:g}"))
    print(f"{gn}: worst share of the bar {max(r[4] for r in rows):.3f}")
    assert not ch.failures(rows)
    zr = ch.zero_rows([(dense["ids"], dense["mask"])], geom)
    for g in (g_reg, g_b):
        assert not g["encoder.embeddings.word_embeddings.weight"][zr].any()


def _regime_b_passes_criterion_e_under_the_loss(gn):
    geom, lossy = GEOMS[gn], lossy_of(gn)
    g_b = ch.grads_loss("regime_b", sd_of(gn), geom, lossy["batches"])[1]
    rows, e_pool = ch.criterion_e(g_b, lossy["reg"][1], lossy["m64"][1], geom)
    print(ch.table(rows, e_pool, f"{gn}: regime_b, in-batch loss"))
    print(f"{gn}: worst share of the bar {max(r[4] for r in rows):.3f}")
    assert not ch.failures(rows)


def test_regime_b_passes_criterion_e_under_the_loss():
    _regime_b_passes_criterion_e_under_the_loss("TINY")


def test_regime_b_passes_criterion_e_under_the_loss_on_deep():
    _regime_b_passes_criterion_e_under_the_loss("DEEP")


def mutated_rows(gn, mutation):
    """(the mutated regime's gradients, criterion E's rows for them): under the loss for last_call_only (only the loss uses the weights more
    than once), under the dense cotangent otherwise"""
    geom, sd = GEOMS[gn], sd_of(gn)
    if mutation == "last_call_only":
        lossy = lossy_of(gn)
        g_m = ch.grads_loss("regime", sd, geom, lossy["batches"], mutation)[1]
        return g_m, ch.criterion_e(g_m, lossy["reg"][1], lossy["m64"][1], geom)[0]
    dense = dense_of(gn)
    _, g_m = ch.grads_cotangent("regime", sd, geom, dense["ids"], dense["mask"], dense["G"], 1.0, mutation)
    return g_m, ch.criterion_e(g_m, dense["g_reg"], dense["g64"], geom)[0]


@pytest.mark.parametrize("gn,mutation", [pytest.param("TINY", m, id=m) for m in TINY_MUTATIONS] + [pytest.param("DEEP", m, id="DEEP-" + m) for m in ch.MUTATIONS])
def test_every_mutation_fails_criterion_e(gn, mutation):
    _, rows = mutated_rows(gn, mutation)
    bad = ch.failures(rows)
    print(f"{gn}: {mutation}: {len(bad)} of {len(rows)} tensors over the bar, up to {max(r[4] for r in rows):.3g} x")
    assert bad


@pytest.mark.parametrize("mutation", ch.MID_MUTATIONS)
def test_two_layers_cannot_show_a_middle_layers_defect(mutation):
    """the blind spot that DEEP closes. A defect in the hand-off from a full layer to a full layer (0 < i < layers - 1) leaves every TINY
    gradient EQUAL to the unmutated regime's, element for element: no test on TINY can see it, whatever its tolerance. On DEEP it fails
    criterion E."""
    assert GEOMS["TINY"]["layers"] == 2 and GEOMS["DEEP"]["layers"] >= 4
    g_m, rows = mutated_rows("TINY", mutation)
    g_reg = dense_of("TINY")["g_reg"]
    assert set(g_m) == set(g_reg)
    differ = [k for k in g_reg if not np.array_equal(g_m[k], g_reg[k])]
    assert not differ and not ch.failures(rows), differ
    _, rows = mutated_rows("DEEP", mutation)
    bad = ch.failures(rows)
    print(f"{mutation}: TINY 0 of {len(g_reg)} tensors differ from the regime's; DEEP {len(bad)} of {len(rows)} over the bar, up to {max(r[4] for r in rows):.3g} x")
    assert bad


# ---- dropout at every site ---------------------------------------------------------------------------------------------------------------------
DROP = (ch.DROP_P, ch.DROP_SEED)
# (geometry, batch, p) of every dense device case of tests/test_encoder_chain_dropout_gpu.py
DROP_DENSE = [(gn, name, ch.DROP_P) for gn in GEOMS for name in ch.BATCHES] + [("TINY", "L48", 0.5)]


@functools.lru_cache(maxsize=None)
def drop_dense_of(gn, name="L48", p=ch.DROP_P):
    """a batch under the fixed cotangent with dropout at every site: the masks, the masked model64 and the masked regime, once"""
    geom, sd = GEOMS[gn], sd_of(gn)
    ids, mask = ch.batch(name, geom)
    G = ch.cotangent(len(ids), geom)
    drop = (p, ch.DROP_SEED, 0)
    emb64, g64 = ch.grads_cotangent("model64", sd, geom, ids, mask, G, drop=drop)
    emb_reg, g_reg = ch.grads_cotangent("regime", sd, geom, ids, mask, G, drop=drop)
    return dict(ids=ids, mask=mask, G=G, drop=drop, masks=ch.dropout_masks(geom, ids, mask, *drop), emb64=emb64, g64=g64, emb_reg=emb_reg, g_reg=g_reg)


@functools.lru_cache(maxsize=None)
def drop_lossy_of(gn):
    geom, sd = GEOMS[gn], sd_of(gn)
    batches = ch.loss_batches(geom)
    return dict(batches=batches, m64=ch.grads_loss("model64", sd, geom, batches, drop=DROP), reg=ch.grads_loss("regime", sd, geom, batches, drop=DROP))


def test_site_of_is_injective_and_fits_a_uint32():
    layers = max(g["layers"] for g in GEOMS.values())
    sites = [ch.site_of(e, 0, "emb") for e in range(len(ch.KEYS))]
    sites += [ch.site_of(e, i, place) for e in range(len(ch.KEYS)) for i in range(layers) for place in ch.PLACES[1:]]
    assert len(sites) == len(set(sites)) == 6 * (3 * layers + 1)
    assert all(0 < s < 2 ** 32 for s in sites)
    # and up to the depth the function admits (roberta-base has 12 layers)
    deep = {ch.site_of(e, i, place) for e in range(len(ch.KEYS)) for i in range(ch.MAX_LAYERS) for place in ch.PLACES if place != "emb" or i == 0}
    assert len(deep) == 6 * (3 * ch.MAX_LAYERS + 1) and max(deep) < 2 ** 32


@pytest.mark.parametrize("gn", list(GEOMS))
def test_every_mask_of_every_test_batch_keeps_and_drops(gn):
    """no site of any device case is trivially all-kept or all-dropped; the factors are 0, the scale, or 1 at positions no token owns; and the
    mapping of dropout_masks, spot-checked against the replica directly: token t of sequence b is packed row cu[b] + t, a CLS row is row b"""
    import dropout_ref
    geom = GEOMS[gn]
    todo = [(ch.batch(name, geom), (p, ch.DROP_SEED, 0)) for g, name, p in DROP_DENSE if g == gn]
    todo += [(b, DROP + (n,)) for n, b in enumerate(ch.loss_batches(geom).values())]
    for (ids, mask), drop in todo:
        T = dropout_ref.threshold(drop[0])
        scale = float(dropout_ref.scale(T))
        masks = ch.dropout_masks(geom, ids, mask, *drop)
        assert len(masks) == 3 * geom["layers"] + 2  # (emb16 is emb)
        for key, m in masks.items():
            assert set(np.unique(m)) <= {0.0, scale, 1.0} and (m == 0).any() and (m == scale).any(), (key, drop)
        lens = mask.sum(1)
        cu = np.concatenate([[0], np.cumsum(lens)])
        b, last = len(lens) - 1, geom["layers"] - 1
        t = int(lens[b]) - 1
        keep = dropout_ref.hidden_keep(int(cu[-1]), geom["hidden"], T, drop[1], ch.site_of(drop[2], 0, "ao"))
        assert np.array_equal(masks["ao", 0][b, t] != 0, keep[cu[b] + t])
        keep = dropout_ref.hidden_keep(len(lens), geom["hidden"], T, drop[1], ch.site_of(drop[2], last, "ff2"))
        assert np.array_equal(masks["ff2", last] != 0, keep)
        for i, mode in ((0, 0), (last, 3)):
            for h in range(geom["heads"]):
                want = dropout_ref.attn_keep(0, np.arange(lens[b]), b * geom["heads"] + h, T, drop[1], ch.site_of(drop[2], i, "attn"))
                assert np.array_equal(masks["attn", i][b, h, 0, :lens[b]] != 0, want), (i, h)


@pytest.mark.parametrize("gn,name,p", [pytest.param(*c, id="-".join(map(str, c))) for c in DROP_DENSE])
def test_dropout_batches_meet_criterion_es_premises(gn, name, p):
    """what a device case needs of its batch: under the masks every compared tensor has a non-zero fp64 gradient, the key bias's is still
    mathematically zero (the rows of dS sum to zero under a probability mask: delta_i = sum_j p_ij dP_ij whatever dP is), unused rows are zero"""
    geom, d = GEOMS[gn], drop_dense_of(gn, name, p)
    sets = [(d["g64"], [(d["ids"], d["mask"])])]
    if (name, p) == ("L48", ch.DROP_P):
        lossy = drop_lossy_of(gn)
        sets.append((lossy["m64"][1], list(lossy["batches"].values())))
    for g64, batches in sets:
        for k in ch.param_names(geom):
            if k not in ch.zero_grad_names(geom):
                assert np.abs(g64[k]).max() > 0, k
        for k in ch.zero_grad_names(geom):
            mine, qb = np.abs(g64[k]).max(), np.abs(g64[k.replace("key", "query")]).max()
            print(f"{gn} {name} p {p}: {k}: max |g64| {mine:.3e}, the query bias's {qb:.3e}")
            assert mine <= 1e-12 * qb
        zr = ch.zero_rows(batches, geom)
        assert zr.any() and not g64["encoder.embeddings.word_embeddings.weight"][zr].any()


@pytest.mark.parametrize("gn,scale", [(gn, s) for gn in GEOMS for s in (1.0, 256.0)])
def test_masked_regime_and_regime_b_pass_criterion_e(gn, scale):
    geom, sd, d = GEOMS[gn], sd_of(gn), drop_dense_of(gn)
    _, g_reg = ch.grads_cotangent("regime", sd, geom, d["ids"], d["mask"], d["G"], scale, drop=d["drop"]) if scale != 1.0 else (None, d["g_reg"])
    emb_b, g_b = ch.grads_cotangent("regime_b", sd, geom, d["ids"], d["mask"], d["G"], scale, drop=d["drop"])
    # regime_b against the regime at its own scale; and the regime under a loss scale against the regime at scale 1
    for who, g, yard in (("regime_b", g_b, g_reg),) + ((("regime", g_reg, d["g_reg"]),) if scale != 1.0 else ()):
        rows, e_pool = ch.criterion_e(g, yard, d["g64"], geom)
        print(ch.table(rows, e_pool, f"{gn}: {who} with dropout, L48, scale {scale:g}"))
        print(f"{gn}: {who} with dropout, scale {scale:g}: worst share of the bar {max(r[4] for r in rows):.3f}")
        assert not ch.failures(rows)
    err = np.abs(d["emb_reg"] - d["emb64"])
    if scale == 1.0:
        print(f"{gn}: masked regime forward against the masked model64: max {err.max():.3e} mean {err.mean():.3e}; regime_b's max {np.abs(emb_b - d['emb64']).max():.3e}")
    assert np.abs(emb_b - d["emb64"]).max() <= 2.0 * err.max()


@pytest.mark.parametrize("gn", list(GEOMS))
def test_masked_regime_b_passes_criterion_e_under_the_loss(gn):
    geom, lossy = GEOMS[gn], drop_lossy_of(gn)
    g_b = ch.grads_loss("regime_b", sd_of(gn), geom, lossy["batches"], drop=DROP)[1]
    rows, e_pool = ch.criterion_e(g_b, lossy["reg"][1], lossy["m64"][1], geom)
    print(ch.table(rows, e_pool, f"{gn}: regime_b with dropout, in-batch loss"))
    print(f"{gn}: regime_b with dropout, in-batch loss: worst share of the bar {max(r[4] for r in rows):.3f}")
    assert not ch.failures(rows)


@pytest.mark.parametrize("gn,mutation", [(gn, m) for gn in GEOMS for m in ch.DROP_MUTATIONS])
def test_every_dropout_mutation_fails_criterion_e(gn, mutation):
    geom, d = GEOMS[gn], drop_dense_of(gn)
    _, g_m = ch.grads_cotangent("regime", sd_of(gn), geom, d["ids"], d["mask"], d["G"], 1.0, mutation, drop=d["drop"])
    rows = ch.criterion_e(g_m, d["g_reg"], d["g64"], geom)[0]
    bad = ch.failures(rows)
    print(f"{gn}: {mutation}: {len(bad)} of {len(rows)} tensors over the bar, up to {max(r[4] for r in rows):.3g} x")
    assert bad


@pytest.mark.parametrize("gn", list(GEOMS))
def test_all_ones_masks_are_no_dropout(gn):
    """the masked models under factors of one everywhere: the regime returns the unmasked gradients element for element (x * 1 and a second
    rounding of a rounded value change nothing); so does regime_b in its embeddings, and in its gradients up to what two plain runs of it
    differ by (torch's fp32 index backward on the CPU adds a table row's terms in no fixed order: 2^-20 of the tensor's largest element is
    sixteen fp32 ulps of it); the masked fp64 model, which runs the last layer on the CLS rows alone, to 1e-12"""
    geom, sd, dense, d = GEOMS[gn], sd_of(gn), dense_of(gn), drop_dense_of(gn)
    ones = ch.ones_masks(d["masks"])
    emb1, g1 = ch.grads_cotangent("regime", sd, geom, d["ids"], d["mask"], d["G"], drop=ones)
    assert np.array_equal(emb1, dense["emb_reg"]) and all(np.array_equal(g1[k], dense["g_reg"][k]) for k in g1)
    emb1, g1 = ch.grads_cotangent("regime_b", sd, geom, d["ids"], d["mask"], d["G"], drop=ones)
    emb0, g0 = ch.grads_cotangent("regime_b", sd, geom, d["ids"], d["mask"], d["G"])
    assert np.array_equal(emb1, emb0) and all(np.abs(g1[k] - g0[k]).max() <= 2.0 ** -20 * np.abs(g0[k]).max() for k in g0)
    emb1, g1 = ch.grads_cotangent("model64", sd, geom, d["ids"], d["mask"], d["G"], drop=ones)
    assert np.abs(emb1 - dense["emb64"]).max() <= 1e-12
    for k in ch.param_names(geom):
        if k not in ch.zero_grad_names(geom):
            assert np.abs(g1[k] - dense["g64"][k]).max() <= 1e-12 * np.abs(dense["g64"][k]).max(), k
    # and the masks do something: the masked fp64 model is another function
    assert np.abs(d["emb64"] - dense["emb64"]).max() > 1e-2
