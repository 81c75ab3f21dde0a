"""GPU (-m gpu): the retriever encoder's backward as ONE chain of the package's differentiable functions -- packed_embedding_layer_norm,
packed_linear, packed_self_attention, packed_layer_norm, mhop_loss_outputs -- composed as the product's forward in its default mode
(residual_fp32 = 2; csrc/mdr_encoder_trunk.inl), on oracle.seeded.TINY. The host side is tests/encoder_chain_ref.py.

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
import embedding_grad_ref as eref
import encoder_chain_ref as ch
import layernorm_grad_ref as nref
import linear_grad_ref as lref
import mhop_loss_ref
from encoder_chain_dev import E_, EPS, F, GEOM, H, NH, PAD, Chain, _np, _p, check_e, grads_np, params, poison, same_bits  # noqa: F401
from oracle import seeded
from oracle import trunk_rows_oracle as tr

pytestmark = pytest.mark.gpu

TINY_BAR = (6e-3, 1.2e-3)  # tests/test_encoder_gpu.py's TOL["tiny"]: max and mean |error| of the embeddings against fp64
CONFIGS = [("L160", 1.0), ("L160", 256.0), ("L48", 1.0), ("L48", 256.0)]


# ---- B: one stage's raw backward, re-run on the taped tensors, inside the derived bound ------------------------------------------------------
def _f32(shape):
    return torch.empty(shape, dtype=torch.float32, device="cuda")


def rerun(c, rec):
    """-> (device results, {input key: dx}, {param name: gradient}, {output: share of the bound}); asserts the bound"""
    from multihop_dense_retrieval_amd import attention, embedding, layernorm, linear
    kind, lab, g = rec["kind"], rec["label"], rec["g"]
    P = c.P
    shares, fails = {}, []

    def ratio(name, got, r, bnd, wr=lref.worst_ratio):
        worst, at = wr(got, r, bnd)
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
        ratio("dg", _np(dg), *rb["dg"], wr=nref.worst_ratio)
        ratio("db", _np(db), *rb["db"], wr=nref.worst_ratio)
        res = ({"dx16": dx16, "dx32": dx32, "dg": dg, "db": db}, {"x": dx16, "res": dx32}, {nm + ".weight": dg, nm + ".bias": db})
    elif kind == "attn":
        qkv, mode = rec["ins"]["qkv"].detach(), rec["mode"]
        dctx = g["ctx"].to(torch.float16).contiguous()
        dq = attention.attention_backward(qkv, dctx, c.cu, NH, c.L, mode)
        cu = _np(c.cu)
        d_np = _np(dctx) if mode == 3 else _np(dctx)[:c.T]
        ratio("dqkv", _np(dq)[:c.T], *aref.reference_and_bound(_np(qkv)[:c.T], d_np, cu, NH, mode), wr=aref.worst_ratio)
        res = ({"dqkv": dq}, {"qkv": dq}, {})
    elif kind == "emb":
        names = [E_ + n for n in ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias")]
        word, pos, typ, wt = (P[n].detach() for n in names[:4])
        dy16, dy2 = g["y16"].to(torch.float16).contiguous(), g["y32"].to(torch.float32).contiguous()
        plan = embedding.embedding_plan(c.ids, c.src, c.pid, c.total, c.cap, GEOM["vocab"], GEOM["max_pos"], PAD)
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
    assert n >= 16
    if param_grads_used_once:
        seen = set()
        for lab, (_, _, pg, _) in st.items():
            for name, gr in pg.items():
                assert same_bits(c.P[name].grad, gr.reshape(c.P[name].shape).contiguous()), (lab, name)
                seen.add(name)
        assert seen == set(ch.param_names()), set(ch.param_names()) ^ seen


# ---- the runs, each made once ----------------------------------------------------------------------------------------------------------------
_RUNS = {}


def dense_run(name, scale, with_poison=False):
    ids, mask = ch.batch(name)
    P = params()
    if with_poison:
        poison()
    c = Chain(P, ids, mask)
    G = torch.from_numpy(ch.cotangent(len(ids)) * np.float32(scale)).cuda()
    if with_poison:
        poison()
    c.out.backward(G)
    torch.cuda.synchronize()
    return c


def loss_run(with_poison=False):
    from multihop_dense_retrieval_amd import criterions
    P = params()
    batches = ch.loss_batches()
    if with_poison:
        poison()
    cs = {k: Chain(P, *batches[k]) for k in ch.KEYS}
    loss = criterions.mhop_loss_outputs({k: cs[k].out for k in ch.KEYS}, types.SimpleNamespace(fp16=True))
    if with_poison:
        poison()
    loss.backward()
    torch.cuda.synchronize()
    return cs, loss, P


def run(key):
    if key not in _RUNS:
        _RUNS[key] = loss_run() if key == "loss" else dense_run(*key)
    return _RUNS[key]


_HOST = {}


def host_dense(name):
    """model64 and the regime at scales 1 and 2^8 on the CPU, once per batch"""
    if name not in _HOST:
        sd = ch.state_dict()
        ids, mask = ch.batch(name)
        G = ch.cotangent(len(ids))
        emb64, g64 = ch.grads_cotangent("model64", sd, GEOM, ids, mask, G)
        _HOST[name] = dict(emb64=emb64, g64=g64, reg={s: ch.grads_cotangent("regime", sd, GEOM, ids, mask, G, s)[1] for s in (1.0, 256.0)})
    return _HOST[name]


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ch.BATCHES))
def test_a_forward_is_the_products_up_to_the_fp16_head(name):
    from multihop_dense_retrieval_amd import _lib, retriever
    t0 = time.time()
    c = run((name, 1.0))
    ids, mask = ch.batch(name)
    cfg = retriever.RobertaConfig(vocab_size=GEOM["vocab"], hidden_size=H, num_hidden_layers=GEOM["layers"], num_attention_heads=NH, intermediate_size=F)
    m = retriever.RobertaRetriever(cfg, None)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded.make_state_dict(ch.WEIGHT_SEED, GEOM).items()})
    m.to("cuda").eval()
    assert int(m.residual_fp32) == 2
    prod = m.encode_q(torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda(), None)
    chain, e64 = _np(c.out).astype(np.float64), host_dense(name)["emb64"]
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
    _lib.check(L_.mdr_test_gemm_f16(_p(cls16), _p(w16), _p(c.P["project.0.bias"].detach()), B, None, H, H, _p(pre), 3, 0, 0, _lib.current_stream_ptr()))
    _lib.check(L_.mdr_test_layernorm(_p(pre), 0, None, None, B, None, H, _p(c.P["project.1.weight"].detach()), _p(c.P["project.1.bias"].detach()), EPS,
                                     _p(out16), _p(out32), 0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    biteq = same_bits(out32, prod.detach().to(torch.float32))
    print(f"FWD {name}: mean |chain - encode_q| {d_cp.mean():.3e} (max {d_cp.max():.3e}); chain - model64 mean {d_c64.mean():.3e} max {d_c64.max():.3e}; "
          f"encode_q - model64 mean {d_p64.mean():.3e} max {d_p64.max():.3e}; the chain in front of project.0 + the product's fp32 head == encode_q bit for bit: {biteq}")
    assert biteq, "the chain in front of project.0 does not compose to the product's forward"
    assert d_cp.mean() <= d_c64.mean() and d_cp.mean() <= d_p64.mean()
    for d in (d_c64, d_p64):
        assert d.max() <= TINY_BAR[0] and d.mean() <= TINY_BAR[1]
    print(f"WALL a {name} {time.time() - t0:.2f} s")


# ---- B and C ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", CONFIGS)
def test_bc_stages_within_derived_bounds_and_wiring_bit_for_bit(name, scale):
    from multihop_dense_retrieval_amd import layernorm
    t0 = time.time()
    c = run((name, scale))
    st = stages(c)
    torch.cuda.synchronize()
    check_wiring(c, st)
    # the fp32 stream of the last full layer: zero but for the CLS rows, which hold the tail's first LayerNorm's dx32
    last = GEOM["layers"] - 1
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
    print(f"WALL bc {name} scale {scale:g} {time.time() - t0:.2f} s")


def test_bc_loss_stages_and_the_six_encode_sums():
    t0 = time.time()
    cs, loss, P = run("loss")
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
    for name in ch.param_names():
        acc = per[order[0]][name].reshape(P[name].shape).clone()
        for k in order[1:]:
            acc = acc + per[k][name].reshape(P[name].shape)
        assert same_bits(P[name].grad, acc.contiguous()), name
    print(f"WALL bc loss {time.time() - t0:.2f} s")


def test_c_two_whole_runs_give_the_same_bits():
    t0 = time.time()
    a, b = run(("L160", 1.0)), dense_run("L160", 1.0)
    for k in a.P:
        assert same_bits(a.P[k].grad, b.P[k].grad), k
    assert same_bits(a.out, b.out)
    _, loss_a, Pa = run("loss")
    _, loss_b, Pb = loss_run()
    assert same_bits(loss_a.reshape(1), loss_b.reshape(1))
    for k in Pa:
        assert same_bits(Pa[k].grad, Pb[k].grad), k
    print(f"WALL c {time.time() - t0:.2f} s")


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------
def test_d_unwritten_rows_are_never_read():
    t0 = time.time()
    run(("L160", 1.0))
    poison()  # the premise: what torch.empty hands out after the seeding is NaN, in the chain's own sizes
    probe = [torch.empty(s, dtype=d, device="cuda") for s, d in (((1280, H), torch.float16), ((1280, 3 * H), torch.float16), ((8, H), torch.float32))]
    assert all(bool(torch.isnan(t).all()) for t in probe), "the allocator did not hand the seeded blocks out: this test would show nothing"
    del probe
    for name in ch.BATCHES:
        a, b = run((name, 1.0)), dense_run(name, 1.0, with_poison=True)
        for k in a.P:
            assert torch.isfinite(b.P[k].grad).all(), (name, k)
            assert same_bits(a.P[k].grad, b.P[k].grad), (name, k)
    _, _, Pa = run("loss")
    _, loss_b, Pb = loss_run(with_poison=True)
    assert torch.isfinite(loss_b)
    for k in Pa:
        assert torch.isfinite(Pb[k].grad).all(), k
        assert same_bits(Pa[k].grad, Pb[k].grad), k
    print(f"WALL d {time.time() - t0:.2f} s")


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", CONFIGS)
def test_e_gradients_against_the_fp64_model(name, scale):
    t0 = time.time()
    c, h = run((name, scale)), host_dense(name)
    check_e(grads_np(c.P, scale), h["reg"][scale], h["g64"], [ch.batch(name)], f"{name} scale {scale:g}")
    print(f"WALL e {name} scale {scale:g} {time.time() - t0:.2f} s")


def test_e_loss_gradients_against_the_fp64_model():
    t0 = time.time()
    _, loss, P = run("loss")
    sd, batches = ch.state_dict(), ch.loss_batches()
    l64, g64, _, _ = ch.grads_loss("model64", sd, GEOM, batches)
    lreg, g_reg, _, _ = ch.grads_loss("regime", sd, GEOM, batches)
    print(f"E loss: device {float(loss.detach()):.6f} regime {lreg:.6f} model64 {l64:.6f}")
    check_e(grads_np(P), g_reg, g64, list(batches.values()), "in-batch loss")
    print(f"WALL e loss {time.time() - t0:.2f} s")
