"""GPU (-m gpu): mdr_reader_heads_forward / mdr_reader_heads_backward (include/mdr_reader_loss.h) against the fp64 statement of
tests/reader_loss_ref.py, and the whole brick -- CLS gather, linear.packed_linear (the pooler), reader_loss.reader_heads, reader_loss.qa_loss,
backward() -- against the gradients the reference's own QAModel.forward produced in fp32 (tests/golden/reader_loss_ref.npz).

Bounds: the helper's DERIVED windows (fp32 accumulation in any order; an fp16 rounding may flip only where a boundary lies inside the fp32
error). On the exact grid every product and sum is exact in fp32, so the logits are the helper's bits.

Shapes of the backward: SINGLE_ROW (B L <= 256: one token row per wave of the token kernel) and SEVERAL_ROWS (whole batches of L = 512 at
H = 1024 and 128, the smallest with two and three rows per wave); the comments at the lists say why each is there."""
import os

import numpy as np
import pytest
import torch

import reader_loss_ref as ref
from guarded import Guarded, dev
from oracle import fp

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reader_loss_ref.npz")
SLACK = 3  # rows of h16 / d_h behind cu[B]: never read, never written


def device_case(c):
    rows, cu = ref.pack(c["seq"], c["lens"])
    T, H = rows.shape
    h = torch.zeros((T + SLACK, H), dtype=torch.float16, device="cuda")
    h[:T] = dev(rows.astype(np.float16))
    W, b = ref.heads_params16(c["P"])
    return {"h": h, "T": T, "cu": dev(cu), "dense": dev(c["dense"].astype(np.float16)), "pmask": dev(c["pmask"]),
            "offs": dev(c["offs"]) if c["offs"] is not None else None, "w16": dev(W[[0, 1, 2, 3]].astype(np.float16)), "b32": dev(b.astype(np.float32))}


def forward(c, d):
    from multihop_dense_retrieval_amd import _lib, reader_loss
    B, L = c["pmask"].shape
    NS = c["offs"].shape[1] if c["offs"] is not None else 0
    H = c["seq"].shape[2]
    out = {"start": Guarded(B, (L,), torch.float16, 2, 2, name="start"), "end": Guarded(B, (L,), torch.float16, 2, 2, name="end"),
           "rank": Guarded(B, (), torch.float16, 2, 2, name="rank")}
    if NS:
        out["sp"] = Guarded(B, (NS,), torch.float16, 2, 2, name="sp")
    p = _lib.ptr
    _lib.call(reader_loss.lib().mdr_reader_heads_forward, p(d["h"]), p(d["cu"]), p(d["dense"]), p(d["pmask"]), p(d["offs"]), B, L, NS, H, p(d["w16"]), p(d["b32"]),
              out["start"].ptr(), out["end"].ptr(), out["rank"].ptr(), out["sp"].ptr() if NS else None, dev=d["h"].device)
    torch.cuda.synchronize()
    return {k: o.checked() for k, o in out.items()}


OUT_SHAPES = lambda B, H: {"d_dense": (B, (H,), torch.float16), "dw_qa": (2, (H,), torch.float32), "db_qa": (2, (), torch.float32),  # noqa: E731
                           "dw_sp": (1, (H,), torch.float32), "db_sp": (1, (), torch.float32), "dw_rank": (1, (H,), torch.float32), "db_rank": (1, (), torch.float32)}


def backward(c, d, g, old=None):
    """one mdr_reader_heads_backward into guarded buffers; old: {name: array} of values to accumulate into (accumulate = 1)"""
    from multihop_dense_retrieval_amd import _lib, reader_loss
    B, L = c["pmask"].shape
    NS = c["offs"].shape[1] if c["offs"] is not None else 0
    H, T = c["seq"].shape[2], d["T"]
    L_ = reader_loss.lib()
    out = {"d_h": Guarded(T + SLACK, (H,), torch.float16, 1, 1, name="d_h")}
    for k, (n, tail, dt) in OUT_SHAPES(B, H).items():
        if NS or not k.endswith("_sp"):
            out[k] = Guarded(n, tail, dt, 16, 16, init=None if old is None else old[k], name=k)  # 16 guard rows keep the [.., H] buffers 16-byte aligned
    need = int(L_.mdr_reader_heads_backward_workspace_bytes(B, L, H))
    ws = _lib.workspace(need, d["h"].device)
    p = _lib.ptr
    gd = {k: dev(np.asarray(v, np.float16)) if v is not None else None for k, v in g.items()}
    _lib.call(L_.mdr_reader_heads_backward, p(d["h"]), p(d["cu"]), p(d["dense"]), p(d["pmask"]), p(d["offs"]), B, L, NS, H, T + SLACK, p(d["w16"]), p(gd["start"]),
              p(gd["end"]), p(gd["rank"]), p(gd.get("sp")), out["d_h"].ptr(), out["d_dense"].ptr(), out["dw_qa"].ptr(), out["db_qa"].ptr(),
              out["dw_sp"].ptr() if NS else None, out["db_sp"].ptr() if NS else None, out["dw_rank"].ptr(), out["db_rank"].ptr(), 0 if old is None else 1,
              p(ws), need, dev=d["h"].device)
    torch.cuda.synchronize()
    res = {k: o.checked(valid=T if k == "d_h" else None) for k, o in out.items()}
    res["d_h"] = ref.unpack(res["d_h"][:T], c["lens"], L)
    return res


def random_grads(c, seed, scale=8.0):
    rng = np.random.default_rng(seed)
    B, L = c["pmask"].shape
    g = {"start": ref.h16(scale * rng.standard_normal((B, L))), "end": ref.h16(scale * rng.standard_normal((B, L))), "rank": ref.h16(scale * rng.standard_normal(B))}
    g["sp"] = ref.h16(scale * rng.standard_normal(c["offs"].shape)) if c["offs"] is not None else None
    return g


def test_forward_on_an_exact_grid_is_bit_equal():
    c = ref.make_heads_case(4, 40, 5, 128, 3, lens=[40, 33, 30, 25], exact=True)
    got = forward(c, device_case(c))
    val, win = ref.heads_forward(c["seq"], c["dense"], c["lens"], c["pmask"], c["offs"], c["P"])
    for k in ("start", "end", "sp"):  # exact fp32 sums: the one fp16 rounding is the helper's
        assert fp.same_bits(got[k], val[k].astype(np.float16)), k
    assert np.isneginf(got["start"]).any() and np.isfinite(got["start"]).any() and np.isfinite(got["sp"]).all()
    # rank sits behind tanh. The grid's dense values are multiples of 2: tanh is 1 in fp32 from |x| = 10 on, and below that no fp16 rounding
    # boundary lies within 4 ulp of tanh(x) (asserted), so pooled16 is fixed; its 11-bit values times multiples of 1/8 sum exactly in fp32
    t = np.tanh(c["dense"])
    assert (ref.win16(t, 4 * fp.U32 * np.abs(t))[1] == 0).all()
    assert fp.same_bits(got["rank"], val["rank"].astype(np.float16))


@pytest.mark.parametrize("H,B,L,NS", [(128, 3, 33, 4), (768, 5, 40, 5), (1024, 4, 64, 30), (256, 1, 17, 0), (1024, 6, 512, 30)])
def test_forward_within_the_derived_bound(H, B, L, NS):
    """(the last case: rows of L = 512 logits at the reader's width, the first of SEVERAL_ROWS below)"""
    c = ref.make_heads_case(B, L, NS, H, 5)
    got = forward(c, device_case(c))
    val, win = ref.heads_forward(c["seq"], c["dense"], c["lens"], c["pmask"], c["offs"], c["P"])
    for k, g in got.items():
        inf = np.isneginf(val[k])
        assert np.array_equal(np.isneginf(g), inf), k
        fp.assert_within(np.where(inf, 0, g), np.where(inf, 0, val[k]), win[k], f"forward {k}")


# T = 127, 128, 129 packed rows; B in {1, 4, 5}; ragged rows; NS = 30 > 2 duplicate markers and padded offsets that name the CLS row; B L / 4 chunks
# of the token split (rows per chunk = 4 at these sizes: 32 .. 64 chunks, more than the 16 strands of the second stage)
SINGLE_ROW = [(128, 1, 127, 0, [127]), (128, 4, 40, 5, [40, 33, 30, 25]), (768, 5, 40, 5, [40, 20, 31, 17, 21]), (1024, 4, 64, 30, None), (256, 5, 50, 1, None)]
# With B L <= 256 a chunk of the token split is 4 rows: each of the four waves of reader_heads_token_grad_kernel walks ONE row, its fp32 fma
# chains a0 / a1 / a2 hold one term and the `i += 4` loop body runs once -- an accumulator that is overwritten instead of added to passes all
# of the above. The chunk grows only with B L (1024 chunks at the most, fewer at H = 1024 where the partials' byte cap binds first), so the
# smallest shapes with several rows per wave are whole batches of L = 512, the reader's own row length: at H = 1024, B = 3 is the smallest
# batch with 8 rows per chunk (2 per wave, 192 chunks) and B = 6 the smallest with 12 (3 per wave, 256 chunks, NS = 30 markers); at H = 128,
# the other end of the widths, B = 9 is the smallest with 8 (576 chunks, 36 for each of the sixteen strands of the second stage). Ragged rows of
# the helper's own lengths: a wave's rows lie in different sequences and some are skipped as padding.
SEVERAL_ROWS = [(1024, 6, 512, 30, None), (1024, 3, 512, 5, None), (128, 9, 512, 5, None)]
BACKWARD = SINGLE_ROW + SEVERAL_ROWS


@pytest.mark.parametrize("H,B,L,NS,lens", BACKWARD, ids=[f"H{s[0]}-B{s[1]}-L{s[2]}-NS{s[3]}" for s in BACKWARD])
def test_backward_within_the_derived_bound(H, B, L, NS, lens):
    from multihop_dense_retrieval_amd import reader_loss
    c = ref.make_heads_case(B, L, NS, H, 7, lens=lens)
    ws_bytes = int(reader_loss.lib().mdr_reader_heads_backward_workspace_bytes(B, L, H))
    assert ws_bytes >= 3 * H * 4 * 8  # several chunks
    if (H, B, L, NS, lens) in SEVERAL_ROWS:  # the workspace is [S][3][H] floats: S chunks of at least 8 rows, two rows or more for every wave
        assert ws_bytes % (3 * H * 4) == 0
        S = ws_bytes // (3 * H * 4)
        assert S * 8 <= (B * L + 7) // 8 * 8, (S, B * L)
        live = np.arange(L)[None, :] < np.asarray(c["lens"])[:, None]
        assert B * L % S == 0 and (live.reshape(S, B * L // S).sum(axis=1) >= 8).any(), "no chunk holds two live rows for every wave"
    if lens is not None:
        assert sum(lens) in (127, 128, 129)
    if NS >= 2:
        assert (c["offs"][:, 0] == c["offs"][:, 1]).any() and (c["offs"] == 0).any()
    d, g = device_case(c), random_grads(c, 8)
    got = backward(c, d, g)
    want, bound = ref.heads_backward(c["seq"], c["dense"], c["lens"], c["pmask"], c["offs"], c["P"], g)
    assert set(got) == set(want)
    worst = {k: fp.assert_within(got[k].reshape(want[k].shape), want[k], bound[k], f"backward {k}") for k in want}
    print(f"H={H} B={B} L={L} NS={NS}", "worst |got - ref| / bound:", {k: f"{v:.3f}" for k, v in worst.items()})
    live = np.arange(L)[None, :] < np.asarray(c["lens"])[:, None]
    unread = live & (c["pmask"] != 1)
    if NS:
        for b in range(B):
            unread[b, c["offs"][b][(c["offs"][b] >= 0) & (c["offs"][b] < c["lens"][b])]] = False
    assert unread.any() and (got["d_h"][unread] == 0).all()  # rows no head reads are written as 0
    again = backward(c, d, g)
    for k in got:
        assert fp.same_bits(got[k], again[k]), k


def test_accumulate_adds_into_the_buffers():
    H, B, L, NS = 128, 4, 40, 5
    c = ref.make_heads_case(B, L, NS, H, 9)
    d, g = device_case(c), random_grads(c, 10)
    rng = np.random.default_rng(11)
    old = {k: (50.0 * rng.standard_normal((n,) + tail)).astype(np.float32) for k, (n, tail, dt) in OUT_SHAPES(B, H).items() if dt == torch.float32}
    old["d_dense"] = None
    got = backward(c, d, g, old)
    want, bound = ref.heads_backward(c["seq"], c["dense"], c["lens"], c["pmask"], c["offs"], c["P"], g)
    for k, o in old.items():
        if o is not None:
            w = want[k].reshape(o.shape) + o
            fp.assert_within(got[k], w, bound[k].reshape(o.shape) + fp.U32 * np.abs(w), f"accumulate {k}")  # the old value enters last: one more fp32 add
    for k in ("d_h", "d_dense"):
        fp.assert_within(got[k], want[k], bound[k], f"accumulate {k}")


@pytest.mark.parametrize("case", ["B1_sp", "B5_sp", "B5_nosp"])
def test_the_whole_brick_against_the_reference(case):
    """CLS gather -> packed_linear (the pooler) -> reader_heads -> qa_loss -> backward() on packed ragged rows, with a loss scale of 64.
    (a) Every gradient is inside the helper's O1 bound, evaluated on the device's own forward activations (which are themselves inside the
    forward windows), with the errors of the incoming gradients carried along.
    (b) Against the reference's fp32 numbers the only difference is fp16 rounding. On any path from the loss to a leaf there are at most eight
    fp16 roundings of relative size 2^-11 (input, weight, score or dense, pooled, the loss gradient, a contraction's result, the CLS add, the
    bias), and a logit's own rounding, 2^-11 |x| absolute, enters the softmax through the numerator and the lse; so the norm-wise
    difference of a gradient tensor is at most 2^-11 (8 + 2 max|x|) of the golden's norm, and the loss differs by at most 2^-11 max|x| times the
    sum of its terms' sensitivities (|d term / d x| <= 1 per cross entropy side and per BCE, weighted as the loss weights them)."""
    from multihop_dense_retrieval_amd import linear, reader_loss
    z = np.load(GOLD)
    P = {k[6:]: z[k] for k in z.files if k.startswith("param.")}
    has_sp = case.endswith("_sp")
    if not has_sp:
        P["sp.weight"] = P["sp.bias"] = None
    batch = {k: z[f"{case}.{k}"] for k in ("paragraph_mask", "starts", "ends", "label", "sent_offsets", "sent_labels")}
    seq, lens, spw, g0 = z["seq"][z[f"{case}.rows"]], z[f"{case}.lens"], float(z[f"{case}.sp_weight"].reshape(-1)[0]), 64.0
    B, L, H = seq.shape
    gold = {"seq": z[f"{case}.grad.seq"]}
    for k, v in P.items():
        if v is not None:
            key = f"{case}.grad.{k}"
            gold[k] = z[key] if key in z.files else z[f"{case.replace('nosp', 'sp')}.grad.{k}"]
    rows, cu = ref.pack(seq, lens)
    h16 = dev(rows.astype(np.float16)).requires_grad_(True)
    cu_d = dev(cu)
    params = {k: dev(v).requires_grad_(True) for k, v in P.items() if v is not None}
    tb = {k: dev(v) for k, v in batch.items()}
    cls = h16[cu_d[:-1].to(torch.int64)]
    dense16 = linear.packed_linear(cls, params["pooler.dense.weight"], params["pooler.dense.bias"])
    out = reader_loss.reader_heads(h16, dense16, cu_d, tb, {k: v for k, v in params.items() if not k.startswith("pooler.")})
    loss = reader_loss.qa_loss(out["start_logits"], out["end_logits"], out["rank_score"], out["sp_score"], tb, spw)
    (loss * g0).sum().backward()
    torch.cuda.synchronize()
    np_ = lambda t: None if t is None else t.detach().float().cpu().numpy().astype(np.float64)  # noqa: E731
    fwd = {"dense": np_(dense16), "start": np_(out["start_logits"]), "end": np_(out["end_logits"]), "rank": np_(out["rank_score"]), "sp": np_(out["sp_score"])}
    own = ref.chain(seq, lens, batch, P, g0, spw)
    for k, v in fwd.items():  # the forward, inside its windows
        if v is not None:
            inf = np.isneginf(own["forward"][0][k])
            assert np.array_equal(np.isneginf(v.reshape(inf.shape)), inf), k
            fp.assert_within(np.where(inf, 0, v.reshape(inf.shape)), np.where(inf, 0, own["forward"][0][k]), own["forward"][1][k], f"{case} forward {k}")
    r = ref.chain(seq, lens, batch, P, g0, spw, forward=fwd)
    got = {"seq": ref.unpack(np_(h16.grad), lens, L)}
    got.update({k: np_(v.grad) for k, v in params.items()})
    assert abs(float(loss.item()) - r["loss"]) <= r["loss_bound"]
    worst = {k: fp.assert_within(got[k].reshape(r["grads"][k].shape), r["grads"][k], r["bounds"][k], f"{case} {k}") for k in r["grads"]}
    xmax = max(np.abs(v[np.isfinite(v)]).max() for k, v in fwd.items() if v is not None and k != "dense")
    # qa_outputs.bias is the sum of a softmax gradient over its row, which cancels to 0 in exact arithmetic (the golden holds fp32 noise there): its
    # own norm is no scale, so it is held against the sum of the magnitudes it adds, from the helper's formula on the same scores
    sg = ref.loss_and_grads({"start": fwd["start"], "end": fwd["end"], "rank": fwd["rank"].reshape(-1), "sp": fwd["sp"], "starts": batch["starts"],
                             "ends": batch["ends"], "label": batch["label"], "sent_offsets": batch["sent_offsets"], "sent_labels": batch["sent_labels"]},
                            1.0, spw, o1=False)["grads"]
    scale = {k: np.linalg.norm(v) for k, v in gold.items()}
    scale["qa_outputs.bias"] = np.linalg.norm([np.abs(sg["start"]).sum(), np.abs(sg["end"]).sum()])
    rel = {k: np.linalg.norm(got[k].reshape(gold[k].shape) / g0 - gold[k]) / scale[k] for k in gold}
    print(case, "worst / O1 bound:", {k: f"{v:.3f}" for k, v in worst.items()}, "norm-wise against the fp32 golden:", {k: f"{v:.2e}" for k, v in rel.items()},
          "allowed", f"{fp.H16 * (8 + 2 * xmax):.2e}")
    for k, v in rel.items():
        assert v <= fp.H16 * (8 + 2 * xmax), (k, v)
    label = batch["label"].reshape(-1)
    terms = 2 * B + B + (spw * (batch["sent_offsets"] * label[:, None]).sum() if has_sp else 0.0)
    assert abs(float(loss.item()) - float(z[f"{case}.loss"][0])) <= fp.H16 * xmax * terms + r["loss_bound"]
