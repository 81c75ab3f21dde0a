"""GPU (-m gpu): the encoder chain of tests/test_encoder_chain_gpu.py with the reference's training dropout at EVERY site -- behind the embedding
LayerNorm (packed_dropout(y32, ..., rows=total, also16=True)), on the probabilities of both attention forms (dropout=(p, seed, site)), and on
the outputs of attention.output.dense and output.dense in front of their residual LayerNorms (rows = total on full layers, rows = None on the B
CLS rows of the last layer) -- on oracle.seeded.TINY and DEEP, batches L160 (the ring attention path) and L48, loss scales 1 and 2^8. p = 0.1
(T = 26) throughout, one TINY L48 case at p = 0.5. Every call's site is encoder_chain_ref.site_of(encode, layer, place); the host side
(masks from the replica of tests/dropout_ref.py, the masked fp64 model, the masked regime) is tests/encoder_chain_ref.py, and
tests/test_encoder_chain_host.py holds it on the CPU first.

A0 dropout=(0.001, ...) (T = 0) gives the bits of dropout=None in the embeddings and in every parameter gradient.
A  the chain's embeddings against the masked fp64 model; the bar is twice the host regime's own max and mean distance to that model.
B  every taped stage re-run on the tensors it saw and the gradient autograd delivered (test_encoder_chain_gpu.rerun): a dropout call bit for bit
   against x * m in numpy from the replica's mask, both directions, the also16 pair and its summed gradient, rows behind `total` exactly
   zero; attention with dropout, forward and backward, inside dropout_ref.reference_and_bound under that call's masks; every other stage as
   before, the embedding backward now with dy16 = None. No new tolerance.
C  wiring bit for bit (check_wiring: a dropout's hooked output gradient is its consumer's re-run dx, its re-run dx is what its producer's hook
   saw), the six-encode sums in autograd's order, two whole runs the same bits, another seed other bits in every parameter gradient.
D  the allocator seeded with NaN blocks before the forward and before the backward: every gradient finite and bit-equal.
E  criterion E against the masked fp64 model, the masked regime as yardstick: the bar is 2 max(e_reg, e_pool), from the host.
F  the overflow contract through the chain: +Inf planted at a DROPPED position of the gradient entering a hidden dropout's backward reaches
   the Linear's weight gradient as a non-finite value (the mask is a factor: 0 x Inf = NaN).

Every check prints its figures (`SHARE`, `FWD`, `E ...`) before it asserts; profiles/encoder_grad_chain.md holds them.
"""
import time
import types

import numpy as np
import pytest
import torch

import dropout_ref as dref
import encoder_chain_ref as ch
import mhop_loss_ref
from encoder_chain_dev import Chain, _np, check_e, grads_np, params, poison, same_bits
from test_encoder_chain_gpu import BC_DEEP, CONFIGS, GEOMS, cases, check_wiring, stages

pytestmark = pytest.mark.gpu

P, SEED = ch.DROP_P, ch.DROP_SEED
HALF = ("L48", 1.0, 0.5)  # the one case at p = 0.5 (T = 128)


def pcases(configs_tiny, configs_deep, half=True):
    """cases() with p = 0.1 behind every config, and the TINY L48 case at p = 0.5"""
    return cases([c + (P,) for c in configs_tiny] + ([HALF] if half else []), [c + (P,) for c in configs_deep])


# ---- the runs, each made once ----------------------------------------------------------------------------------------------------------------
_RUNS, _HOST = {}, {}


def dense_run(gn, name, scale, p=P, seed=SEED, with_poison=False, plant=None):
    """one encode with dropout=(p, seed, 0) (p None: dropout=None) under the dense cotangent. plant: (label of a taped stage, output key, row,
    column) -- that element of the gradient arriving at that output is set to +Inf"""
    geom = GEOMS[gn]
    ids, mask = ch.batch(name, geom)
    W = params(geom)
    if with_poison:
        poison(geom=geom)
    c = Chain(W, ids, mask, geom=geom, dropout=None if p is None else (p, seed, 0))
    if plant is not None:
        label, key, row, col = plant

        def inf_at(g):
            g = g.clone()
            g[row, col] = float("inf")
            return g
        [r for r in c.tape if r["label"] == label][0]["outs"][key].register_hook(inf_at)
    G = torch.from_numpy(ch.cotangent(len(ids), geom) * np.float32(scale)).cuda()
    if with_poison:
        poison(geom=geom)
    c.out.backward(G)
    torch.cuda.synchronize()
    return c


def loss_run(gn, seed=SEED, with_poison=False):
    from multihop_dense_retrieval_amd import criterions
    geom = GEOMS[gn]
    W = params(geom)
    batches = ch.loss_batches(geom)
    if with_poison:
        poison(geom=geom)
    cs = {k: Chain(W, *batches[k], geom=geom, dropout=(P, seed, n)) for n, k in enumerate(ch.KEYS)}
    loss = criterions.mhop_loss_outputs({k: cs[k].out for k in ch.KEYS}, types.SimpleNamespace(fp16=True))
    if with_poison:
        poison(geom=geom)
    loss.backward()
    torch.cuda.synchronize()
    return cs, loss, W


def run(*key):
    """run("TINY", "L160", 1.0, 0.1) or run("DEEP", "loss")"""
    if key not in _RUNS:
        _RUNS[key] = loss_run(key[0]) if key[1] == "loss" else dense_run(*key)
    return _RUNS[key]


def host_dense(gn, name, p=P):
    """the masked model64 and the masked regime at scales 1 and 2^8 on the CPU, once per geometry, batch and rate"""
    if (gn, name, p) not in _HOST:
        t0 = time.time()
        geom = GEOMS[gn]
        sd = ch.state_dict(geom)
        ids, mask = ch.batch(name, geom)
        G = ch.cotangent(len(ids), geom)
        drop = (p, SEED, 0)
        emb64, g64 = ch.grads_cotangent("model64", sd, geom, ids, mask, G, drop=drop)
        reg = {s: ch.grads_cotangent("regime", sd, geom, ids, mask, G, s, drop=drop) for s in (1.0, 256.0)}
        _HOST[gn, name, p] = dict(emb64=emb64, g64=g64, emb_reg=reg[1.0][0], reg={s: r[1] for s, r in reg.items()})
        print(f"WALL host references with dropout {gn} {name} p {p} {time.time() - t0:.2f} s")
    return _HOST[gn, name, p]


def host_loss(gn):
    if (gn, "loss") not in _HOST:
        t0 = time.time()
        geom = GEOMS[gn]
        sd, batches = ch.state_dict(geom), ch.loss_batches(geom)
        _HOST[gn, "loss"] = dict(batches=batches, m64=ch.grads_loss("model64", sd, geom, batches, drop=(P, SEED)),
                                 reg=ch.grads_loss("regime", sd, geom, batches, drop=(P, SEED)))
        print(f"WALL host references with dropout {gn} loss {time.time() - t0:.2f} s")
    return _HOST[gn, "loss"]


# ---- A0 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gn,name", cases(list(ch.BATCHES), ["L160"]))
def test_a0_a_rate_that_rounds_to_zero_gives_the_bits_of_no_dropout(gn, name):
    from multihop_dense_retrieval_amd import dropout
    assert dropout.threshold(0.001) == 0
    a, b = dense_run(gn, name, 1.0, p=None), dense_run(gn, name, 1.0, p=0.001)
    assert a.dropout is None and b.dropout is not None
    # both attention forms and the hidden calls are made and hand their input on; the embedding's call is not made (below)
    assert not [r for r in a.tape + b.tape if r["kind"] == "drop"]
    assert same_bits(a.out, b.out)
    for k in a.P:
        assert same_bits(a.P[k].grad, b.P[k].grad), k


@pytest.mark.parametrize("gn", list(GEOMS))
def test_a0_the_embeddings_fp16_copy_is_a_rounding_of_its_own(gn):
    """why the chain makes no embedding dropout call at T = 0. embed_ln_kernel rounds the UNROUNDED LayerNorm value to fp16 once; the also16
    dropout call returns fp16(y32), a second rounding of the fp32 value. They differ only where y32 lies exactly between two fp16 values (the
    first rounding landed on a tie), by one fp16 ulp: with packed_dropout(y32, T = 0, also16=True) in the graph the QKV Linear would see other
    bits than without dropout. Held here: wherever the two differ, y32 is such a midpoint and the kernel's copy is a neighbour."""
    from multihop_dense_retrieval_amd import dropout
    c = run(gn, "L160", 1.0, P)
    emb = [r for r in c.tape if r["label"] == "emb"][0]
    y16, y32 = _np(emb["outs"]["y16"])[:c.T], _np(emb["outs"]["y32"])[:c.T]
    T0 = dropout.dropout_rows(emb["outs"]["y32"].detach(), 0, SEED, 1, c.total, None, True)
    assert same_bits(T0[0][:c.T], emb["outs"]["y32"].detach()[:c.T]) and np.array_equal(_np(T0[1])[:c.T], y32.astype(np.float16))
    twice = y32.astype(np.float16)
    differ = y16 != twice
    d_mine, d_twice = np.abs(y16.astype(np.float64) - y32), np.abs(twice.astype(np.float64) - y32)
    print(f"A0 {gn}: the embedding's y16 != fp16(y32) at {int(differ.sum())} of {differ.size} elements")
    assert (d_mine[differ] == d_twice[differ]).all() and (d_mine[differ] > 0).all(), "a difference that is not a tie of the second rounding"


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gn,name", cases(list(ch.BATCHES), list(ch.BATCHES)))
def test_a_forward_against_the_masked_fp64_model(gn, name):
    c, host = run(gn, name, 1.0, P), host_dense(gn, name)
    d_r64 = np.abs(host["emb_reg"] - host["emb64"])
    d_c64 = np.abs(_np(c.out).astype(np.float64) - host["emb64"])
    bar = (2.0 * d_r64.max(), 2.0 * d_r64.mean())
    print(f"FWD dropout {gn} {name}: regime - model64 mean {d_r64.mean():.3e} max {d_r64.max():.3e} (CPU); bar max {bar[0]:.3e} mean {bar[1]:.3e}; "
          f"chain - model64 mean {d_c64.mean():.3e} max {d_c64.max():.3e}")
    assert d_c64.max() <= bar[0] and d_c64.mean() <= bar[1]


# ---- B and C ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gn,name,scale,p", pcases(CONFIGS, BC_DEEP))
def test_bc_stages_within_derived_bounds_and_wiring_bit_for_bit(gn, name, scale, p):
    t0 = time.time()
    c = run(gn, name, scale, p)
    st = stages(c)
    torch.cuda.synchronize()
    check_wiring(c, st)
    nl = GEOMS[gn]["layers"]
    # site discipline: every call of the encode drew at a site of its own, the one site_of names for its layer and place
    sites = {r["label"]: r["drop"][2] for r in c.tape if r.get("drop") is not None}
    want = {"emb.drop": ch.site_of(0, 0, "emb")}
    for i in range(nl):
        want.update({f"L{i}.attn": ch.site_of(0, i, "attn"), f"L{i}.ao.drop": ch.site_of(0, i, "ao"), f"L{i}.ff2.drop": ch.site_of(0, i, "ff2")})
    assert sites == want and len(set(sites.values())) == 3 * nl + 1
    # the embedding's backward saw a gradient on y32 alone, and the CLS tail's dropout calls ran on B rows without a row count
    emb = [r for r in c.tape if r["label"] == "emb"][0]
    assert "y16" not in emb["g"] and "y32" in emb["g"]
    for place in ("ao", "ff2"):
        r = [r for r in c.tape if r["label"] == f"L{nl - 1}.{place}.drop"][0]
        assert r["rows"] is None and r["ins"]["x"].shape[0] == c.B
    print(f"WALL bc dropout {gn} {name} scale {scale:g} p {p} {time.time() - t0:.2f} s")


@pytest.mark.parametrize("gn", list(GEOMS))
def test_bc_loss_stages_and_the_six_encode_sums(gn):
    t0 = time.time()
    cs, loss, W = run(gn, "loss")
    emb = {k: _np(cs[k].out) for k in ch.KEYS}
    ref = mhop_loss_ref.loss_and_grads(emb, o1=True)
    got = {k: _np(cs[k].tape[-1]["g"]["y32"]) for k in ch.KEYS}
    assert mhop_loss_ref.violations(ref, float(loss.detach()), got) == []
    per, sites = {}, []
    for k in ch.KEYS:
        st = stages(cs[k])
        check_wiring(cs[k], st, param_grads_used_once=False)
        per[k] = {}
        for _, (_, _, pg, _) in st.items():
            per[k].update(pg)
        sites += [r["drop"][2] for r in cs[k].tape if r.get("drop") is not None]
    assert len(sites) == len(set(sites)) == 6 * (3 * GEOMS[gn]["layers"] + 1), "two calls of one step share a site"
    order = list(reversed(ch.KEYS))  # autograd runs the node made last first
    for name in ch.param_names(GEOMS[gn]):
        acc = per[order[0]][name].reshape(W[name].shape).clone()
        for k in order[1:]:
            acc = acc + per[k][name].reshape(W[name].shape)
        assert same_bits(W[name].grad, acc.contiguous()), name
    print(f"WALL bc dropout {gn} loss {time.time() - t0:.2f} s")


@pytest.mark.parametrize("gn", list(GEOMS))
def test_c_two_whole_runs_give_the_same_bits_and_another_seed_other_bits(gn):
    a, b, other = run(gn, "L160", 1.0, P), dense_run(gn, "L160", 1.0), dense_run(gn, "L160", 1.0, seed=SEED + 1)
    assert same_bits(a.out, b.out) and not same_bits(a.out, other.out)
    for k in a.P:
        assert same_bits(a.P[k].grad, b.P[k].grad), k
        # (under a FIXED cotangent G, project.1.bias's gradient is G's column sum: no mask reaches it. Under the loss below it moves too)
        assert same_bits(a.P[k].grad, other.P[k].grad) == (k == "project.1.bias"), (k, "another seed left a gradient's bits alone")
    _, loss_a, Wa = run(gn, "loss")
    _, loss_b, Wb = loss_run(gn)
    _, loss_o, Wo = loss_run(gn, seed=SEED ^ (1 << 40))
    assert same_bits(loss_a.reshape(1), loss_b.reshape(1)) and not same_bits(loss_a.reshape(1), loss_o.reshape(1))
    for k in Wa:
        assert same_bits(Wa[k].grad, Wb[k].grad), k
        assert not same_bits(Wa[k].grad, Wo[k].grad), (k, "another seed left a gradient's bits alone")


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gn", list(GEOMS))
def test_d_unwritten_rows_are_never_read(gn):
    geom = GEOMS[gn]
    H = geom["hidden"]
    run(gn, "L160", 1.0, P)
    poison(geom=geom)  # the premise: what torch.empty hands out after the seeding is NaN, in the chain's own sizes
    probe = [torch.empty(s, dtype=d, device="cuda") for s, d in (((1280, H), torch.float16), ((1280, 3 * H), torch.float16), ((8, H), torch.float32))]
    print(f"D dropout {gn}: share of NaN in the probes {[round(float(torch.isnan(t).float().mean()), 4) for t in probe]}; reserved "
          f"{torch.cuda.memory_reserved() >> 20} MiB, allocated {torch.cuda.memory_allocated() >> 20} MiB")
    assert all(bool(torch.isnan(t).all()) for t in probe), "the allocator did not hand the seeded blocks out: this test would show nothing"
    del probe
    for name in ch.BATCHES:
        a, b = run(gn, name, 1.0, P), dense_run(gn, name, 1.0, with_poison=True)
        for k in a.P:
            assert torch.isfinite(b.P[k].grad).all(), (name, k)
            assert same_bits(a.P[k].grad, b.P[k].grad), (name, k)
    _, _, Wa = run(gn, "loss")
    _, loss_b, Wb = loss_run(gn, with_poison=True)
    assert torch.isfinite(loss_b)
    for k in Wa:
        assert torch.isfinite(Wb[k].grad).all(), k
        assert same_bits(Wa[k].grad, Wb[k].grad), k


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gn,name,scale,p", pcases(CONFIGS, CONFIGS))
def test_e_gradients_against_the_masked_fp64_model(gn, name, scale, p):
    geom = GEOMS[gn]
    c, h = run(gn, name, scale, p), host_dense(gn, name, p)
    check_e(grads_np(c.P, scale), h["reg"][scale], h["g64"], [ch.batch(name, geom)], f"dropout p {p} {gn} {name} scale {scale:g}", geom)


@pytest.mark.parametrize("gn", list(GEOMS))
def test_e_loss_gradients_against_the_masked_fp64_model(gn):
    _, loss, W = run(gn, "loss")
    h = host_loss(gn)
    (l64, g64, _, _), (lreg, g_reg, _, _) = h["m64"], h["reg"]
    print(f"E dropout {gn} loss: device {float(loss.detach()):.6f} regime {lreg:.6f} model64 {l64:.6f}")
    check_e(grads_np(W), g_reg, g64, list(h["batches"].values()), f"dropout {gn} in-batch loss", GEOMS[gn])


# ---- F ---------------------------------------------------------------------------------------------------------------------------------------
def test_f_an_overflow_at_a_dropped_position_reaches_the_weight_gradient():
    """DESIGN.md 20's contract through the chain. The position is found on the host: a token row and a column of layer 0's attention.output
    dropout that the mask DROPS. +Inf there, in the gradient entering that dropout's backward, times the factor 0 is NaN: the Linear's weight
    gradient must not be finite, and without the plant it is."""
    gn, name = "TINY", "L48"
    geom = GEOMS[gn]
    _, mask = ch.batch(name, geom)
    keep = dref.hidden_keep(int(mask.sum()), geom["hidden"], dref.threshold(P), SEED, ch.site_of(0, 0, "ao"))
    row, col = (int(v) for v in np.argwhere(~keep)[len(np.argwhere(~keep)) // 2])
    assert not keep[row, col] and row < int(mask.sum())
    w = "encoder.encoder.layer.0.attention.output.dense.weight"
    clean = run(gn, name, 1.0, P)
    assert torch.isfinite(clean.P[w].grad).all()
    c = dense_run(gn, name, 1.0, plant=("L0.ao.drop", "y", row, col))
    g = c.P[w].grad
    print(f"F: +Inf planted at dropped ({row}, {col}) of L0.ao.drop's output gradient: {int((~torch.isfinite(g)).sum())} non-finite elements of {w}, "
          f"all in row {col}: {bool(torch.isfinite(g[torch.arange(g.shape[0], device='cuda') != col]).all())}")
    assert not torch.isfinite(g).all(), "a drop hid an overflow"
