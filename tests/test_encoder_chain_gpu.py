"""GPU (-m gpu): the retriever encoder's backward as ONE chain of the package's differentiable functions -- packed_embedding_layer_norm,
packed_linear, packed_self_attention, packed_layer_norm, mhop_loss_outputs -- composed as the product's forward in its default mode
(residual_fp32 = 2; csrc/mdr_encoder_trunk.inl), on oracle.seeded.TINY and on oracle.seeded.DEEP. The host side is tests/encoder_chain_ref.py.

TINY has two layers: the first one and the last one, which runs on the CLS rows alone. DEEP has four, the smallest depth in which a full layer
hands its fp32 stream and its fp16 copy to another full layer: there the gradient on the stream is dense (on TINY it is zero but for the B CLS
rows) and meets the next QKV Linear's dense fp16 dx in the layer's second LayerNorm backward. tests/test_encoder_chain_host.py shows that a
defect in that hand-off leaves every TINY gradient unchanged. The TINY cases keep the ids they had; DEEP's are `DEEP-...` and `..._on_deep`.

A  forward: the chain's embeddings against RobertaRetriever.encode_q and the fp64 model.
B  every taped function, on the device tensors it really saw and the upstream gradient autograd really delivered: the raw backward re-run,
   every element inside the DERIVED bound of tests/{embedding,layernorm,linear,attention}_grad_ref.py and tests/mhop_loss_ref.py. No new
   tolerance. Rows at or behind `total` are excluded by index, nothing else.
C  wiring, bit for bit: autograd's parameter gradients are the re-run stages' (the three slices of cat(Wq, Wk, Wv) too), an activation's hooked
   gradient is its consumer's re-run dx, the CLS gather's backward, the six-encode sums in autograd's order, and two whole runs agree.
D  unwritten rows: the caching allocator is seeded with NaN blocks before the forward and before the backward; every gradient stays finite
   and keeps its bits.
E  end to end: criterion E of tests/encoder_chain_ref.py against the fp64 model, the yardstick being the reference regime's own error.

What mode 2 makes of two items one might expect here. The fp16 copy of the last full layer's output has ONE consumer, the QKV Linear: the CLS
rows' residual is taken from the fp32 stream, so the CLS rows' gradient lands on h32 (fp32, B rows of it non-zero) and h16 receives the QKV
Linear's dx alone. No fp16 activation of the chain has two consumers. The sum "QKV dx on every row + the CLS rows' gradient on B rows" is
therefore checked where it arises (h32, against autograd's index backward), and gather_cls_backward is held against autograd for the same
sum on the chain's own tensors (the QKV Linear's dx and the CLS rows' gradient rounded to fp16), as `--do_train` under residual_fp32 = 0 needs it.

Excluded from criterion E, by the argument in tests/encoder_chain_ref.py: attention.self.key.bias (gradient mathematically zero; checked under B,
absolutely). word_embeddings rows that own no token, and padding_idx's row: equality with zero instead of a ratio.

Every check prints its figures (`SHARE`, `FWD`, `E ...`) before it asserts; profiles/encoder_grad_chain.md holds them.
"""
import time
import types

import numpy as np
import pytest
import torch

import attention_grad_ref as aref
import dropout_ref as dref
import embedding_grad_ref as eref
import encoder_chain_ref as ch
import layernorm_grad_ref as nref
import linear_grad_ref as lref
import mhop_loss_ref
from encoder_chain_dev import E_, Chain, _np, check_e, grads_np, params, poison, same_bits
from multihop_dense_retrieval_amd._lib import ptr
from oracle import fp, seeded
from oracle import trunk_rows_oracle as tr

pytestmark = pytest.mark.gpu

GEOMS = {"TINY": seeded.TINY, "DEEP": seeded.DEEP}
TINY_BAR = (6e-3, 1.2e-3)  # tests/test_encoder_gpu.py's TOL["tiny"]: max and mean |error| of the embeddings against fp64. TINY's alone.
CONFIGS = [("L160", 1.0), ("L160", 256.0), ("L48", 1.0), ("L48", 256.0)]
BC_DEEP = [("L160", 1.0), ("L48", 256.0)]  # both attention kernels and both scales once; E runs all four


def cases(configs_tiny, configs_deep):
    """(geometry name, *config): TINY's ids are what they were before the second geometry came"""
    one = lambda c: c if isinstance(c, tuple) else (c,)  # noqa: E731
    return ([pytest.param("TINY", *one(c), id="-".join(str(v) for v in one(c))) for c in configs_tiny]
            + [pytest.param("DEEP", *one(c), id="-".join(["DEEP"] + [str(v) for v in one(c)])) for c in configs_deep])


# ---- B: one stage's raw backward, re-run on the taped tensors, inside the derived bound ------------------------------------------------------
def _f32(shape):
    return torch.empty(shape, dtype=torch.float32, device="cuda")


def rerun(c, rec):
    """-> (device results, {input key: dx}, {param name: gradient}, {output: share of the bound}); asserts the bound"""
    from multihop_dense_retrieval_amd import attention, dropout, embedding, layernorm, linear
    kind, lab, g = rec["kind"], rec["label"], rec["g"]
    P, geom = c.P, c.geom
    H, NH, EPS, PAD = geom["hidden"], geom["heads"], geom["ln_eps"], geom["pad_id"]
    shares, fails = {}, []

    def ratio(name, got, r, bnd):
        worst, at = fp.worst_ratio(got, r, bnd)
        shares[name] = worst
        if not worst <= 1.0:
            fails.append(f"{name}: worst |err| / bound {worst:.3f} at {at}")

    if kind == "linear":
        x, w, b, rows = rec["ins"]["x"].detach(), rec["w"].detach(), rec["b"].detach(), rec["rows"]
        w16, dy = w.to(torch.float16).contiguous(), g["y"].to(torch.float16).contiguous()
        pre = None
        if rec["gelu"]:
            with torch.no_grad():
                pre = linear.packed_linear(x, w, b, False, rows)
        dx, dw, db = linear.linear_backward(x, w16, dy, pre, rows, True, _f32(w.shape), _f32(w.shape[0]), False)
        m = c.T if rows is not None else x.shape[0]
        rb = lref.reference_and_bound(_np(x), _np(w16), _np(dy), _np(pre), m)
        ratio("dx", _np(dx)[:m], *rb["dx"])
        ratio("dw", _np(dw), *rb["dw"])
        ratio("db", _np(db), *rb["db"])
        names = rec["names"]
        n = w.shape[0] // len(names)
        pg = {}
        for j, nm in enumerate(names):
            pg[nm + ".weight"], pg[nm + ".bias"] = dw[j * n:(j + 1) * n], db[j * n:(j + 1) * n]
        res = ({"dx": dx, "dw": dw, "db": db}, {"x": dx}, pg)
    elif kind == "ln":
        x, r32, rows, nm = rec["ins"]["x"].detach(), rec["ins"]["res"], rec["rows"], rec["name_"]
        r32 = None if r32 is None else r32.detach()
        wt = P[nm + ".weight"].detach()
        dy16 = None if "y16" not in g else g["y16"].to(torch.float16).contiguous()
        dy2 = None if "y32" not in g else g["y32"].to(torch.float32).contiguous()
        dx16, dx32, dg, db = layernorm.layer_norm_backward(x, r32, dy16, dy2, wt, EPS, rows, True, r32 is not None, _f32(wt.shape), _f32(wt.shape), False)
        m = c.T if rows is not None else x.shape[0]
        rb = nref.reference_and_bound(_np(x), _np(r32), _np(dy16), _np(dy2), _np(wt), EPS, m)
        shares["dx16_not_rne"] = tr.assert_f16(_np(dx16)[:m], *rb["dx"], lab + " dx16")
        if dx32 is not None:
            shares["dx32"] = tr.assert_f32(_np(dx32)[:m], *rb["dx"], lab + " dx32")
        ratio("dg", _np(dg), *rb["dg"])
        ratio("db", _np(db), *rb["db"])
        res = ({"dx16": dx16, "dx32": dx32, "dg": dg, "db": db}, {"x": dx16, "res": dx32}, {nm + ".weight": dg, nm + ".bias": db})
    elif kind == "attn":
        qkv, mode = rec["ins"]["qkv"].detach(), rec["mode"]
        dctx = g["ctx"].to(torch.float16).contiguous()
        cu = _np(c.cu)
        d_np = _np(dctx) if mode == 3 else _np(dctx)[:c.T]
        if rec.get("drop") is None:
            dq = attention.attention_backward(qkv, dctx, c.cu, NH, c.L, mode)
            ratio("dqkv", _np(dq)[:c.T], *aref.reference_and_bound(_np(qkv)[:c.T], d_np, cu, NH, mode))
        else:  # the training forward too: the chain is the first place it runs at these shapes
            dq = attention.attention_dropout_backward(qkv, dctx, c.cu, NH, c.L, mode, *rec["drop"])
            ctx_r, ctx_b, dq_r, dq_b = dref.reference_and_bound(_np(qkv)[:c.T], d_np, cu, NH, mode, dref.attn_masks(cu, NH, mode, *rec["drop"]))
            ctx = _np(rec["outs"]["ctx"])
            ratio("ctx", ctx if mode == 3 else ctx[:c.T], ctx_r, ctx_b)
            ratio("dqkv", _np(dq)[:c.T], dq_r, dq_b)
        res = ({"dqkv": dq}, {"qkv": dq}, {})
    elif kind == "drop":  # bits, both directions: x * m in numpy from the replica's mask; nothing written at or behind the valid count
        x, rows, (T, seed, site) = rec["ins"]["x"].detach(), rec["rows"], rec["drop"]
        M, N = x.shape
        valid = c.T if rows is not None else M
        m = np.where(dref.hidden_keep(M, N, T, seed, site), dref.scale(T), np.float32(0))
        also16 = "y32" in rec["outs"]
        y = _np(rec["outs"]["y32" if also16 else "y"])
        want = (_np(x).astype(np.float32) * m).astype(y.dtype)
        same = [np.array_equal(fp.bits(y[:valid]), fp.bits(want[:valid])), not fp.bits(y[valid:]).any()]
        g32 = g.get("y32" if also16 else "y")
        g16 = g.get("y16")
        assert g32 is not None or g16 is not None, (lab, "no gradient reached a dropout's output")
        if also16:
            y16 = _np(rec["outs"]["y16"])
            same += [np.array_equal(fp.bits(y16[:valid]), fp.bits(want[:valid].astype(np.float16))), not fp.bits(y16[valid:]).any()]
            gz = torch.zeros(x.shape, dtype=torch.float32, device="cuda") if g32 is None else g32.contiguous()
            a16 = None if g16 is None else g16.to(torch.float16).contiguous()
            dx = dropout.dropout_rows(gz, T, seed, site, rows, a16, False)
            want_dx = (_np(gz) + (0 if a16 is None else _np(a16).astype(np.float32))) * m
        else:
            gz = g32.to(x.dtype).contiguous()
            dx = dropout.dropout_rows(gz, T, seed, site, rows, None, False)
            want_dx = (_np(gz).astype(np.float32) * m).astype(_np(gz).dtype)
        same += [np.array_equal(fp.bits(_np(dx)[:valid]), fp.bits(want_dx[:valid])), not fp.bits(_np(dx)[valid:]).any()]
        dropped = float((m[:valid] == 0).mean())
        shares.update(dropped=dropped, bits_equal=all(same))
        if not all(same):
            fails.append(f"y, rows behind the count of y, (y16, its rows,) dx, rows behind the count of dx -- bit-equal: {same}")
        if T and not 0.0 < dropped < 1.0:
            fails.append("the mask keeps or drops everything")
        res = ({"dx": dx}, {"x": dx}, {})
    elif kind == "emb":
        names = [E_ + n for n in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias")]
        word, pos, typ, wt = (P[n].detach() for n in names[:4])
        # (with dropout behind it the embedding's own fp16 copy has no consumer: dy16 is None, the other branch of the backward)
        dy16, dy2 = None if "y16" not in g else g["y16"].to(torch.float16).contiguous(), g["y32"].to(torch.float32).contiguous()
        plan = embedding.embedding_plan(c.ids, c.src, c.pid, c.total, c.cap, geom["vocab"], geom["max_pos"], PAD)
        outs = [_f32(word.shape), _f32(pos.shape), _f32((H,)), _f32((H,)), _f32((H,)), torch.zeros((c.cap, H), dtype=torch.float32, device="cuda")]
        embedding.embedding_backward(c.ids, c.src, c.pid, c.total, c.cap, word, pos, typ[0], wt, EPS, dy16, dy2, plan, *outs)
        case = dict(ids=c.ids_np, tok_src=_np(c.src), tok_pid=_np(c.pid), total=c.T, word=_np(word), pos=_np(pos), type0=_np(typ[0]), g=_np(wt),
                    dy16=_np(dy16), dy2=_np(dy2), pad_row=PAD)
        got = dict(zip(("dword", "dpos", "dtype0", "dg", "db"), (_np(o) for o in outs[:5])), d=_np(outs[5])[:c.T])
        shares.update(eref.worst_shares(got, eref.reference_and_bound(case, EPS)))
        fails += [f"{k}: worst |err| / bound {v:.3f}" for k, v in shares.items() if not v <= 1.0]
        pg = dict(zip(names, outs[:5]))
        pg[names[2]] = outs[2].reshape(1, H)
        res = (dict(zip(("dword", "dpos", "dtype0", "dg", "db", "d"), outs)), {}, pg)
    elif kind == "gather":  # autograd's own index backward: exact
        src = rec["ins"]["src32"]
        dx = torch.zeros_like(src)
        dx[c.starts] = g["cls32"]
        res = ({}, {"src32": dx}, {})
    else:
        raise AssertionError(kind)
    print(f"SHARE {lab} " + " ".join(f"{k}={v:.4f}" if isinstance(v, float) else f"{k}={v}" for k, v in shares.items()))
    assert not fails, (lab, fails)
    return res + (shares,)


def stages(c):
    """every taped function re-run (B asserted inside): {label: (results, input gradients, parameter gradients, shares)}"""
    return {rec["label"]: rerun(c, rec) for rec in c.tape}


def check_wiring(c, st, param_grads_used_once=True):
    """C for one encode: the hooked gradient of every output that has a consumer equals that consumer's re-run dx, bit for bit (rows in
    front of `total`); with param_grads_used_once, every parameter's .grad equals its stage's re-run result"""
    n = 0
    for rec in c.tape:
        for k, t in rec["outs"].items():
            if t is None:
                continue
            cons = [(r2, k2) for r2 in c.tape for k2, t2 in r2["ins"].items() if t2 is t]
            if not cons:
                assert k not in rec["g"] or rec["label"] == "project.1", (rec["label"], k, "a gradient arrived for an output nobody consumes")
                continue
            assert len(cons) == 1, (rec["label"], k, "two consumers: sum their dx here")  # (none in residual_fp32 = 2)
            r2, k2 = cons[0]
            dx, hooked = st[r2["label"]][1][k2], rec["g"][k]
            m = c.T if t.shape[0] == c.cap else t.shape[0]
            assert same_bits(hooked[:m], dx[:m]), (rec["label"], k, "<-", r2["label"], k2)
            n += 1
    # every output but the last LayerNorm's fp32 one and the head's has one consumer: 2 of the embedding, 9 of a full layer, 10 of the last
    # layer with the gather and project.0 (21 on two layers). With dropout: two more outputs per layer (the dropped copies of both Linears'
    # outputs) and one more of the embedding (its y32 and the dropout's pair, its own y16 having lost its consumer)
    taped_drops = sum(r["kind"] == "drop" for r in c.tape)
    assert taped_drops == (0 if c.dropout is None else 2 * c.geom["layers"] + 1), taped_drops
    assert n == 9 * c.geom["layers"] + 3 + taped_drops, n
    if param_grads_used_once:
        seen = set()
        for lab, (_, _, pg, _) in st.items():
            for name, gr in pg.items():
                assert same_bits(c.P[name].grad, gr.reshape(c.P[name].shape).contiguous()), (lab, name)
                seen.add(name)
        assert seen == set(ch.param_names(c.geom)), set(ch.param_names(c.geom)) ^ seen


# ---- the runs, each made once ----------------------------------------------------------------------------------------------------------------
_RUNS = {}


def dense_run(gn, name, scale, with_poison=False):
    geom = GEOMS[gn]
    ids, mask = ch.batch(name, geom)
    P = params(geom)
    if with_poison:
        poison(geom=geom)
    c = Chain(P, ids, mask, geom=geom)
    G = torch.from_numpy(ch.cotangent(len(ids), geom) * np.float32(scale)).cuda()
    if with_poison:
        poison(geom=geom)
    c.out.backward(G)
    torch.cuda.synchronize()
    return c


def loss_run(gn, with_poison=False):
    from multihop_dense_retrieval_amd import criterions
    geom = GEOMS[gn]
    P = params(geom)
    batches = ch.loss_batches(geom)
    if with_poison:
        poison(geom=geom)
    cs = {k: Chain(P, *batches[k], geom=geom) for k in ch.KEYS}
    loss = criterions.mhop_loss_outputs({k: cs[k].out for k in ch.KEYS}, types.SimpleNamespace(fp16=True))
    if with_poison:
        poison(geom=geom)
    loss.backward()
    torch.cuda.synchronize()
    return cs, loss, P


def run(*key):
    """run("TINY", "L160", 1.0) or run("DEEP", "loss")"""
    if key not in _RUNS:
        _RUNS[key] = loss_run(key[0]) if key[1] == "loss" else dense_run(*key)
    return _RUNS[key]


_HOST = {}


def host_dense(gn, name):
    """model64 and the regime at scales 1 and 2^8 on the CPU, once per geometry and batch"""
    if (gn, name) not in _HOST:
        t0 = time.time()
        geom = GEOMS[gn]
        sd = ch.state_dict(geom)
        ids, mask = ch.batch(name, geom)
        G = ch.cotangent(len(ids), geom)
        emb64, g64 = ch.grads_cotangent("model64", sd, geom, ids, mask, G)
        reg = {s: ch.grads_cotangent("regime", sd, geom, ids, mask, G, s) for s in (1.0, 256.0)}
        _HOST[gn, name] = dict(emb64=emb64, g64=g64, emb_reg=reg[1.0][0], reg={s: r[1] for s, r in reg.items()})
        print(f"WALL host references {gn} {name} {time.time() - t0:.2f} s")
    return _HOST[gn, name]


def host_loss(gn):
    """model64 and the regime under the in-batch loss on the CPU, once per geometry"""
    if (gn, "loss") not in _HOST:
        t0 = time.time()
        geom = GEOMS[gn]
        sd, batches = ch.state_dict(geom), ch.loss_batches(geom)
        _HOST[gn, "loss"] = dict(batches=batches, m64=ch.grads_loss("model64", sd, geom, batches), reg=ch.grads_loss("regime", sd, geom, batches))
        print(f"WALL host references {gn} loss {time.time() - t0:.2f} s")
    return _HOST[gn, "loss"]


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gn,name", cases(list(ch.BATCHES), list(ch.BATCHES)))
def test_a_forward_is_the_products_up_to_the_fp16_head(gn, name):
    from multihop_dense_retrieval_amd import _lib, retriever
    t0 = time.time()
    geom = GEOMS[gn]
    H, EPS = geom["hidden"], geom["ln_eps"]
    c = run(gn, name, 1.0)
    ids, mask = ch.batch(name, geom)
    cfg = retriever.RobertaConfig(vocab_size=geom["vocab"], hidden_size=H, num_hidden_layers=geom["layers"], num_attention_heads=geom["heads"],
                                  intermediate_size=geom["ffn"])
    m = retriever.RobertaRetriever(cfg, None)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded.make_state_dict(ch.WEIGHT_SEED, geom).items()})
    m.to("cuda").eval()
    assert int(m.residual_fp32) == 2
    prod = m.encode_q(torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda(), None)
    host = host_dense(gn, name)
    chain, e64 = _np(c.out).astype(np.float64), host["emb64"]
    pr = _np(prod).astype(np.float64)
    d_cp, d_c64, d_p64 = np.abs(chain - pr), np.abs(chain - e64), np.abs(pr - e64)
    # everything in front of project.0: the product's head (bias -> fp32 epilogue, then the LayerNorm of the fp32 sums) on the CHAIN's last fp16
    # activation must give the product's embeddings bit for bit
    cls16 = [r for r in c.tape if r["label"] == "project.0"][0]["ins"]["x"].detach()
    B = cls16.shape[0]
    w16 = c.P["project.0.weight"].detach().to(torch.float16).contiguous()
    pre = torch.zeros((B, H), dtype=torch.float32, device="cuda")
    out16, out32 = torch.zeros((B, H), dtype=torch.float16, device="cuda"), torch.zeros((B, H), dtype=torch.float32, device="cuda")
    L_ = _lib.lib()
    _lib.check(L_.mdr_test_gemm_f16(ptr(cls16), ptr(w16), ptr(c.P["project.0.bias"].detach()), B, None, H, H, ptr(pre), 3, 0, 0, _lib.current_stream_ptr()))
    _lib.check(L_.mdr_test_layernorm(ptr(pre), 0, None, None, B, None, H, ptr(c.P["project.1.weight"].detach()), ptr(c.P["project.1.bias"].detach()), EPS,
                                     ptr(out16), ptr(out32), 0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    biteq = same_bits(out32, prod.detach().to(torch.float32))
    d_r64 = np.abs(host["emb_reg"] - e64)
    # the bar. TINY: the encoder test's. Any other geometry: twice the host regime's own forward distance to the fp64 model, max and mean --
    # criterion E's argument: the device and the regime share the rounding points but not the summation orders, two draws of one size
    bar = TINY_BAR if gn == "TINY" else (2.0 * d_r64.max(), 2.0 * d_r64.mean())
    print(f"FWD {gn} {name}: regime - model64 mean {d_r64.mean():.3e} max {d_r64.max():.3e} (CPU); bar max {bar[0]:.3e} mean {bar[1]:.3e}")
    print(f"FWD {gn} {name}: mean |chain - encode_q| {d_cp.mean():.3e} (max {d_cp.max():.3e}); chain - model64 mean {d_c64.mean():.3e} max {d_c64.max():.3e}; "
          f"encode_q - model64 mean {d_p64.mean():.3e} max {d_p64.max():.3e}; the chain in front of project.0 + the product's fp32 head == encode_q bit for bit: {biteq}")
    assert biteq, "the chain in front of project.0 does not compose to the product's forward"
    assert d_cp.mean() <= d_c64.mean() and d_cp.mean() <= d_p64.mean()
    for d in (d_c64, d_p64):
        assert d.max() <= bar[0] and d.mean() <= bar[1]
    print(f"WALL a {gn} {name} {time.time() - t0:.2f} s")


# ---- B and C ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gn,name,scale", cases(CONFIGS, BC_DEEP))
def test_bc_stages_within_derived_bounds_and_wiring_bit_for_bit(gn, name, scale):
    from multihop_dense_retrieval_amd import layernorm
    t0 = time.time()
    c = run(gn, name, scale)
    st = stages(c)
    torch.cuda.synchronize()
    check_wiring(c, st)
    last = GEOMS[gn]["layers"] - 1
    # a full layer behind a full layer (none on TINY): the gradient on its fp32 stream and the one on its fp16 copy are DENSE, every token row
    # of both is non-zero, and both enter the same LayerNorm backward (check_wiring held them to the next layer's ln1 and qkv re-runs)
    assert (last - 1 > 0) == (gn == "DEEP")
    for i in range(last - 1):
        g = [r for r in c.tape if r["label"] == f"L{i}.ln2"][0]["g"]
        for k in ("y16", "y32"):
            assert k in g, (i, k, "no gradient reached a middle layer's output")
            assert bool(g[k][:c.T].ne(0).any(1).all()), (i, k, "a token row of a middle layer's incoming gradient is all zero")
    # the fp32 stream of the last full layer: zero but for the CLS rows, which hold the tail's first LayerNorm's dx32
    ln2 = [r for r in c.tape if r["label"] == f"L{last - 1}.ln2"][0]
    d32 = ln2["g"]["y32"]
    rest = torch.ones(c.cap, dtype=torch.bool, device="cuda")
    rest[c.starts] = False
    assert not d32[rest].any() and same_bits(d32[c.starts].contiguous(), st[f"L{last}.ln1"][1]["res"])
    assert "y32" not in [r for r in c.tape if r["label"] == f"L{last}.ln2"][0]["g"]  # an unused output: no gradient is materialised
    # gather_cls_backward next to autograd, for the sum the fp16-residual mode needs: the QKV Linear's dx + the CLS rows' gradient in fp16
    dxq = st[f"L{last}.qkv"][1]["x"]
    d_cls = d32[c.starts].to(torch.float16).contiguous()
    t = torch.zeros_like(dxq).requires_grad_(True)
    torch.autograd.backward([t * 1, t[c.starts]], [dxq, d_cls])
    mine = layernorm.gather_cls_backward(d_cls, c.cu, dxq.clone())
    want = dxq.clone()
    want[c.starts] = (dxq[c.starts].float() + d_cls.float()).to(torch.float16)
    assert same_bits(mine[:c.T], want[:c.T]) and same_bits(mine[:c.T], t.grad[:c.T])
    print(f"WALL bc {gn} {name} scale {scale:g} {time.time() - t0:.2f} s")


def _bc_loss_stages_and_the_six_encode_sums(gn):
    t0 = time.time()
    cs, loss, P = run(gn, "loss")
    emb = {k: _np(cs[k].out) for k in ch.KEYS}
    ref = mhop_loss_ref.loss_and_grads(emb, o1=True)
    got = {k: _np(cs[k].tape[-1]["g"]["y32"]) for k in ch.KEYS}
    w = mhop_loss_ref.worst(ref, float(loss.detach()), got)
    print("SHARE loss " + " ".join(f"{k}={v[2]:.4f}" for k, v in w.items()))
    assert mhop_loss_ref.violations(ref, float(loss.detach()), got) == []
    per = {}
    for k in ch.KEYS:
        st = stages(cs[k])
        check_wiring(cs[k], st, param_grads_used_once=False)
        per[k] = {}
        for _, (_, _, pg, _) in st.items():
            per[k].update(pg)
    # autograd runs the node made last first: the fp32 sum starts with the last encode's term
    order = list(reversed(ch.KEYS))
    for name in ch.param_names(GEOMS[gn]):
        acc = per[order[0]][name].reshape(P[name].shape).clone()
        for k in order[1:]:
            acc = acc + per[k][name].reshape(P[name].shape)
        assert same_bits(P[name].grad, acc.contiguous()), name
    print(f"WALL bc {gn} loss {time.time() - t0:.2f} s")


def test_bc_loss_stages_and_the_six_encode_sums():
    _bc_loss_stages_and_the_six_encode_sums("TINY")


def test_bc_loss_stages_and_the_six_encode_sums_on_deep():
    _bc_loss_stages_and_the_six_encode_sums("DEEP")


def _c_two_whole_runs_give_the_same_bits(gn):
    t0 = time.time()
    a, b = run(gn, "L160", 1.0), dense_run(gn, "L160", 1.0)
    for k in a.P:
        assert same_bits(a.P[k].grad, b.P[k].grad), k
    assert same_bits(a.out, b.out)
    _, loss_a, Pa = run(gn, "loss")
    _, loss_b, Pb = loss_run(gn)
    assert same_bits(loss_a.reshape(1), loss_b.reshape(1))
    for k in Pa:
        assert same_bits(Pa[k].grad, Pb[k].grad), k
    print(f"WALL c {gn} {time.time() - t0:.2f} s")


def test_c_two_whole_runs_give_the_same_bits():
    _c_two_whole_runs_give_the_same_bits("TINY")


def test_c_two_whole_runs_give_the_same_bits_on_deep():
    _c_two_whole_runs_give_the_same_bits("DEEP")


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------
def _d_unwritten_rows_are_never_read(gn):
    t0 = time.time()
    geom = GEOMS[gn]
    H = geom["hidden"]
    run(gn, "L160", 1.0)
    poison(geom=geom)  # the premise: what torch.empty hands out after the seeding is NaN, in the chain's own sizes
    probe = [torch.empty(s, dtype=d, device="cuda") for s, d in (((1280, H), torch.float16), ((1280, 3 * H), torch.float16), ((8, H), torch.float32))]
    print(f"D {gn}: share of NaN in the probes {[round(float(torch.isnan(t).float().mean()), 4) for t in probe]}; reserved "
          f"{torch.cuda.memory_reserved() >> 20} MiB, allocated {torch.cuda.memory_allocated() >> 20} MiB")
    assert all(bool(torch.isnan(t).all()) for t in probe), "the allocator did not hand the seeded blocks out: this test would show nothing"
    del probe
    for name in ch.BATCHES:
        a, b = run(gn, name, 1.0), dense_run(gn, name, 1.0, with_poison=True)
        for k in a.P:
            assert torch.isfinite(b.P[k].grad).all(), (name, k)
            assert same_bits(a.P[k].grad, b.P[k].grad), (name, k)
    _, _, Pa = run(gn, "loss")
    _, loss_b, Pb = loss_run(gn, with_poison=True)
    assert torch.isfinite(loss_b)
    for k in Pa:
        assert torch.isfinite(Pb[k].grad).all(), k
        assert same_bits(Pa[k].grad, Pb[k].grad), k
    print(f"WALL d {gn} {time.time() - t0:.2f} s")


def test_d_unwritten_rows_are_never_read():
    _d_unwritten_rows_are_never_read("TINY")


def test_d_unwritten_rows_are_never_read_on_deep():
    _d_unwritten_rows_are_never_read("DEEP")


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gn,name,scale", cases(CONFIGS, CONFIGS))
def test_e_gradients_against_the_fp64_model(gn, name, scale):
    t0 = time.time()
    geom = GEOMS[gn]
    c, h = run(gn, name, scale), host_dense(gn, name)
    check_e(grads_np(c.P, scale), h["reg"][scale], h["g64"], [ch.batch(name, geom)], f"{gn} {name} scale {scale:g}", geom)
    print(f"WALL e {gn} {name} scale {scale:g} {time.time() - t0:.2f} s")


def _e_loss_gradients_against_the_fp64_model(gn):
    t0 = time.time()
    _, loss, P = run(gn, "loss")
    h = host_loss(gn)
    (l64, g64, _, _), (lreg, g_reg, _, _) = h["m64"], h["reg"]
    print(f"E {gn} loss: device {float(loss.detach()):.6f} regime {lreg:.6f} model64 {l64:.6f}")
    check_e(grads_np(P), g_reg, g64, list(h["batches"].values()), f"{gn} in-batch loss", GEOMS[gn])
    print(f"WALL e {gn} loss {time.time() - t0:.2f} s")


def test_e_loss_gradients_against_the_fp64_model():
    _e_loss_gradients_against_the_fp64_model("TINY")


def test_e_loss_gradients_against_the_fp64_model_on_deep():
    _e_loss_gradients_against_the_fp64_model("DEEP")
