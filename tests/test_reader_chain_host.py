"""CPU: the host statements of the answer reader's whole training chain (tests/reader_chain_ref.py) hold each other, on READER3 (three
layers: a first, a middle and a last full layer) and on READER1 (the same widths at one layer, the depth every earlier value test of the
reader's chain ran at).

  - the geometry's keys are reader.expected_state_dict_shapes', the site function is the package's;
  - model64 is Hugging Face's ElectraModel in fp64 (eager attention) with the heads of tests/test_reader_gpu.py::_reference_fn, in its scores
    AND in every gradient: two independent statements, equal to fp64 noise; its loss is reader_loss.host_loss's sequence of torch calls;
  - the heads-and-loss part of `regime` is tests/reader_loss_ref.py's chain (o1 = True), the numpy statement the brick tests rest on, on the
    regime's own final hidden states: forward values, loss and every gradient to fp64 noise;
  - regime_b (fp32 arithmetic, the batch reversed) passes criterion E and the forward criterion against the regime's yardstick, on both
    batches, with and without the sp head, with and without dropout;
  - every mutation fails criterion E on at least one of those configurations: the test stops at the first that shows it, and running this
    file as a script (from the repository root, with it on PYTHONPATH) prints every mutation on every configuration, the table of
    profiles/reader_grad_chain.md;
  - the mutations of ONE_LAYER_BLIND give, on READER1, gradients EQUAL to the unmutated regime's, element for element: no test at one layer
    can see them, whatever its tolerance. That is the gap the three-layer tests close.
Every line prints its figures."""
import functools

import numpy as np
import pytest
import torch

import reader_chain_ref as rc
import reader_loss_ref

GEOMS = {"READER3": rc.READER3, "READER1": rc.READER1}
CONFIGS = [pytest.param(name, sp, drop, id=f"{name}-{'sp' if sp else 'nosp'}-{'drop' if drop else 'plain'}")
           for name in rc.BATCHES for sp in (True, False) for drop in (False, True)]
SCALE = 256.0  # the loss scale of the device cases


@functools.lru_cache(maxsize=None)
def refs(gn, name, sp, drop):
    """model64 and the regime (at the device cases' loss scale) of one configuration, once"""
    geom = GEOMS[gn]
    sd, batch = rc.state_dict(geom, sp), rc.make_batch(name, geom)
    d = rc.DROP if drop else None
    return dict(geom=geom, sd=sd, batch=batch, drop=d, m64=rc.run("model64", sd, geom, batch, drop=d), reg=rc.run("regime", sd, geom, batch, SCALE, drop=d))


def applies(mutation, sp, drop):
    return (drop or mutation not in rc.DROP_ONLY) and (sp or mutation not in rc.SP_ONLY)


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", [True, False])
def test_the_keys_are_the_readers_and_the_sites_the_packages(sp):
    from multihop_dense_retrieval_amd import dropout, reader
    for geom in GEOMS.values():
        want = reader.expected_state_dict_shapes(rc.config(geom), "electra", sp)
        mine = rc.state_dict_shapes(geom, sp)
        assert list(mine) == list(want) and all(tuple(mine[k]) == tuple(want[k]) for k in want)
        sd = rc.state_dict(geom, sp)
        assert list(sd) == list(want) and all(sd[k].shape == tuple(want[k]) and sd[k].dtype == np.float32 for k in want)
    for i in range(rc.READER3["layers"]):
        for place in rc.ch.PLACES:
            if place != "emb" or i == 0:
                assert dropout.site_of(0, i, place) == rc.ch.site_of(0, i, place)
    assert dropout.MAX_LAYERS == rc.ch.MAX_LAYERS and dropout.PLACES == rc.ch.PLACES


@pytest.mark.parametrize("name", list(rc.BATCHES))
def test_the_batches_are_shaped_as_qa_collate_builds_them(name):
    L, lens = rc.BATCHES[name]
    b = rc.make_batch(name)
    assert set(b) == set(rc.INT_KEYS) and b["input_ids"].shape == (len(lens), L) and tuple(b["attention_mask"].sum(1)) == lens
    assert set(b["label"]) == {0, 1} and b["sent_offsets"].shape == (len(lens), rc.NS) and b["starts"].shape == (len(lens), rc.A)
    for r, n in enumerate(lens):
        ids, tt, pm = b["input_ids"][r], b["token_type_ids"][r], b["paragraph_mask"][r]
        seps = np.nonzero(ids[:n] == rc.SEP)[0]
        assert ids[0] == rc.CLS and len(seps) == 2 and seps[1] == n - 1 and not ids[n:].any() and (ids[:n] != 0).all()
        p0 = seps[0] + 1
        assert not tt[:p0].any() and tt[p0:n].all() and not tt[n:].any()  # types 1 behind the first [SEP], 0 on the padding
        assert not pm[:p0].any() and pm[p0:n - 1].all() and not pm[n - 1:].any()
        so = b["sent_offsets"][r]
        k = int((so != 0).sum())
        assert k == min(5, n - 1 - p0) and (so[:k] > 0).all() and not so[k:].any() and (np.diff(so[:k]) > 0).all() and pm[so[:k]].all() and so.max() <= 48
        assert not b["sent_labels"][r, k:].any()
        live = b["starts"][r] >= 0
        assert 1 <= live.sum() <= 3 and live.sum() == 1 + r % rc.A and (b["ends"][r][~live] == -1).all()
        assert pm[b["starts"][r][live]].all() and pm[b["ends"][r][live]].all() and (b["ends"][r][live] >= b["starts"][r][live]).all()
    if name == "R160":
        assert b["sent_labels"].any() and (b["sent_labels"][b["sent_offsets"] != 0] == 0).any()


# ---- model64 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sp", [(n, s) for n in rc.BATCHES for s in (True, False)])
def test_model64_is_hugging_faces_electra_in_fp64(name, sp):
    transformers = pytest.importorskip("transformers")
    from multihop_dense_retrieval_amd import reader_loss
    r = refs("READER3", name, sp, False)
    geom, sd, tb = r["geom"], r["sd"], rc.torch_batch(r["batch"])
    c = rc.config(geom)
    cfg = transformers.ElectraConfig(vocab_size=c.vocab_size, embedding_size=c.embedding_size, hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers,
                                     num_attention_heads=c.num_attention_heads, intermediate_size=c.intermediate_size, hidden_act="gelu",
                                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, max_position_embeddings=c.max_position_embeddings,
                                     type_vocab_size=c.type_vocab_size, layer_norm_eps=c.layer_norm_eps, pad_token_id=c.pad_token_id, attn_implementation="eager")
    enc = transformers.ElectraModel(cfg).double().train()  # (both probabilities are 0: train() changes nothing but is what the gradient is of)
    missing, unexpected = enc.load_state_dict({k[len("encoder."):]: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith("encoder.")}, strict=False)
    assert not [m for m in missing if "position_ids" not in m] and not unexpected, (missing, unexpected)
    W = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items() if not k.startswith("encoder.")}
    h = enc(tb["input_ids"], attention_mask=tb["attention_mask"], token_type_ids=tb["token_type_ids"])[0]
    lo = h @ W["qa_outputs.weight"].T + W["qa_outputs.bias"]
    neg = tb["paragraph_mask"].ne(1)
    start, end = lo[..., 0].masked_fill(neg, -float("inf")), lo[..., 1].masked_fill(neg, -float("inf"))
    pooled = torch.tanh(h[:, 0] @ W["pooler.dense.weight"].T + W["pooler.dense.bias"])
    rank = pooled @ W["rank.weight"].T + W["rank.bias"]
    spv = None
    if sp:
        rep = torch.gather(h, 1, tb["sent_offsets"].unsqueeze(2).expand(-1, -1, h.size(-1)))
        spv = (rep @ W["sp.weight"].T + W["sp.bias"]).squeeze(2)
    hf = {"start_logits": start, "end_logits": end, "rank_score": rank, "sp_score": spv}
    worst = 0.0
    for k in rc.SCORES:
        mine = r["m64"]["scores"][k]
        if hf[k] is None:
            assert mine is None
            continue
        a, b = hf[k].detach().numpy().reshape(mine.shape), mine
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a == -np.inf, b == -np.inf), k
        worst = max(worst, float(np.abs(a[fin] - b[fin]).max()))
    loss = rc.loss_of(start, end, rank, spv, tb, rc.SP_WEIGHT)
    loss.backward()
    g_hf = {"encoder." + k: v.grad for k, v in enc.named_parameters()}
    g_hf.update({k: v.grad for k, v in W.items()})
    assert set(g_hf) == set(sd)
    worst_g = 0.0
    for k, g in r["m64"]["grads"].items():
        a = np.zeros(g.shape) if g_hf[k] is None else g_hf[k].numpy()
        if rc.zero_by_symmetry(k):
            assert np.abs(a).max() <= 1e-12 * np.abs(r["m64"]["grads"][rc.zero_by_symmetry(k)]).max() and np.abs(g).max() <= 1e-12 * np.abs(r["m64"]["grads"][rc.zero_by_symmetry(k)]).max(), k
            continue
        worst_g = max(worst_g, float(np.abs(a - g).max() / np.abs(g).max()))
    print(f"{name} sp {sp}: model64 against Hugging Face in fp64: scores max |diff| {worst:.3e}, loss {float(loss.detach()):.12f} / {r['m64']['loss']:.12f}, "
          f"gradients max |diff| / max |g| {worst_g:.3e}")
    assert worst <= 1e-9 and abs(float(loss.detach()) - r["m64"]["loss"]) <= 1e-9 * abs(float(loss.detach())) and worst_g <= 1e-9
    # the loss formula is host_loss's: the same torch calls in the same order, so on fp32 scores the same bits
    f32 = [None if t is None else t.detach().float() for t in (start, end, rank, spv)]
    assert torch.equal(reader_loss.host_loss(*f32, tb, rc.SP_WEIGHT), rc.loss_of(*f32, tb, rc.SP_WEIGHT).unsqueeze(0).float())
    assert rc.exact_zeros_hold(r["m64"]["grads"], r["batch"], geom)


# ---- the regime's heads and loss are reader_loss_ref's ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sp", [(n, s) for n in rc.BATCHES for s in (True, False)])
def test_the_regimes_heads_and_loss_are_reader_loss_refs_chain(name, sp):
    r = refs("READER3", name, sp, False)
    geom, sd, batch = r["geom"], r["sd"], r["batch"]
    tb = rc.torch_batch(batch)
    tap = {}
    with torch.no_grad():
        rc.forward(rc.leaves(sd), geom, tb, tap=tap)
    seq = tap["h16"]
    assert torch.equal(seq, seq.half().double())  # the regime's final hidden state: fp16 values
    W = rc.leaves(sd)
    x = seq.clone().requires_grad_(True)
    loss, scores = rc.heads_and_loss(W, rc.R(x), tb, rc.SP_WEIGHT)
    (loss * SCALE).backward()
    lens = batch["attention_mask"].sum(1)
    want = reader_loss_ref.chain(seq.numpy(), lens, batch, {k: sd.get(k) for k in ("pooler.dense.weight", "pooler.dense.bias") + reader_loss_ref_keys()},
                                 g0=SCALE, sp_weight=rc.SP_WEIGHT, o1=True)
    fv = want["forward"][0]
    for k, mine in (("start", scores["start_logits"]), ("end", scores["end_logits"]), ("rank", scores["rank_score"]), ("sp", scores["sp_score"])):
        if mine is None:
            assert fv[k] is None
            continue
        assert np.array_equal(mine.detach().numpy().reshape(fv[k].shape), fv[k]), k  # fp16 values on both sides: equal or an fp16 step apart
    loss = loss.detach()
    assert abs(float(loss) - want["loss"]) <= 1e-12 * abs(want["loss"])
    worst = 0.0
    grads = {"seq": x.grad.numpy()}
    grads.update({k: W[k].grad.numpy() for k in want["grads"] if k != "seq"})
    assert set(want["grads"]) == {"seq"} | {k for k in sd if not k.startswith("encoder.")}
    for k, g in want["grads"].items():
        d = np.abs(grads[k].reshape(g.shape) - g).max() / np.abs(g).max()
        worst = max(worst, float(d))
    print(f"{name} sp {sp}: the regime's heads and loss against reader_loss_ref.chain: loss {float(loss):.9f} / {want['loss']:.9f}, "
          f"gradients max |diff| / max |g| {worst:.3e}")
    assert worst <= 1e-12


def reader_loss_ref_keys():
    return ("qa_outputs.weight", "qa_outputs.bias", "rank.weight", "rank.bias", "sp.weight", "sp.bias")


# ---- regime_b --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sp,drop", CONFIGS)
def test_regime_b_passes_criterion_e(name, sp, drop):
    r = refs("READER3", name, sp, drop)
    b = rc.run("regime_b", r["sd"], r["geom"], r["batch"], SCALE, drop=r["drop"])
    rows, e_pool = rc.criterion_e(b["grads"], r["reg"]["grads"], r["m64"]["grads"])
    assert len(rows) == len(r["sd"])
    print(rc.table(rows, e_pool, f"regime_b, {name}, sp {sp}, dropout {drop}"))
    frows, f_pool, same_inf = rc.criterion_fwd(b["scores"], r["reg"]["scores"], r["m64"]["scores"])
    print(rc.table(frows, f_pool, f"FWD regime_b, {name}, sp {sp}, dropout {drop}"))
    print(f"regime_b, {name}, sp {sp}, dropout {drop}: worst share of the bar {max(x[4] for x in rows):.3f}, forward {max(x[4] for x in frows):.3f}; "
          f"loss model64 {r['m64']['loss']:.5f} regime {r['reg']['loss']:.5f} regime_b {b['loss']:.5f}")
    assert not rc.failures(rows) and same_inf and not rc.failures(frows)
    for g in (r["m64"]["grads"], r["reg"]["grads"], b["grads"]):
        assert rc.exact_zeros_hold(g, r["batch"], r["geom"])
    if drop:  # the masks do something, and every site keeps and drops
        plain = refs("READER3", name, sp, False)
        assert abs(plain["m64"]["loss"] - r["m64"]["loss"]) > 1e-2
        masks = rc.dropout_masks(r["geom"], r["batch"], *r["drop"])
        scale = float(rc.dropout_ref.scale(rc.dropout_ref.threshold(rc.DROP[0])))
        for key, m in masks.items():
            assert set(np.unique(m)) <= {0.0, scale, 1.0} and (m == 0).any() and (m == scale).any(), key


# ---- the mutations ---------------------------------------------------------------------------------------------------------------------------
def mutation_rows(mutation, every=False):
    """[(configuration, tensors over the bar, tensors, worst share)] of one mutation: the configurations it applies to, the small batch
    first, up to and including the first on which it fails criterion E; every: all of them (the table of profiles/reader_grad_chain.md)"""
    out = []
    for name in reversed(list(rc.BATCHES)):
        for sp in (True, False):
            for drop in (True, False):
                if not applies(mutation, sp, drop):
                    continue
                r = refs("READER3", name, sp, drop)
                g = rc.run("regime", r["sd"], r["geom"], r["batch"], SCALE, mutation, r["drop"])["grads"]
                rows = rc.criterion_e(g, r["reg"]["grads"], r["m64"]["grads"])[0]
                out.append((f"{name}-{'sp' if sp else 'nosp'}-{'drop' if drop else 'plain'}", len(rc.failures(rows)), len(rows), max(x[4] for x in rows)))
                if out[-1][1] and not every:
                    return out
    return out


@pytest.mark.parametrize("mutation", rc.MUTATIONS)
def test_every_mutation_fails_criterion_e(mutation):
    tried = mutation_rows(mutation)
    print(f"{mutation}: " + "; ".join(f"{c} {n} of {m} over the bar, up to {w:.3g} x" for c, n, m, w in tried))
    assert tried and tried[-1][1]


@pytest.mark.parametrize("mutation", rc.ONE_LAYER_BLIND)
def test_one_layer_cannot_show_a_defect_of_the_loop(mutation):
    """the blind spot READER3 closes: at one layer the loop runs once, and a residual from the wrong layer's stream, an fp16 copy from the
    wrong layer, a dropped hand-over between two full layers or a dropout site that ignores the layer index leaves every gradient EQUAL to
    the unmutated regime's, element for element. On READER3 each fails criterion E (test_every_mutation_fails_criterion_e)."""
    assert rc.READER1["layers"] == 1 and {k: v for k, v in rc.READER1.items() if k != "layers"} == {k: v for k, v in rc.READER3.items() if k != "layers"}
    for name in rc.BATCHES:
        r = refs("READER1", name, True, True)
        m = rc.run("regime", r["sd"], r["geom"], r["batch"], SCALE, mutation, r["drop"])
        differ = [k for k in r["reg"]["grads"] if not np.array_equal(m["grads"][k], r["reg"]["grads"][k])]
        assert set(m["grads"]) == set(r["reg"]["grads"]) and not differ and m["loss"] == r["reg"]["loss"], (name, differ)
    print(f"{mutation}: READER1 0 of {len(r['reg']['grads'])} tensors differ from the regime's, on both batches, with the sp head and dropout")


if __name__ == "__main__":  # every mutation on every configuration it applies to
    for mut in rc.MUTATIONS:
        print(f"| {mut} | " + " | ".join(f"{c}: {n} of {m}, {w:.3g} x" for c, n, m, w in mutation_rows(mut, every=True)) + " |")
