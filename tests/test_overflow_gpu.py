"""GPU (-m gpu): the overflow contract, brick by brick. The host side is tests/overflow_ref.py; tests/test_overflow_host.py holds
the caps of the inputs used here on the references alone.

A  a LIVE non-finite value -- +Inf, -Inf or NaN planted in front of `rows` / `total` -- is DELIVERED to every output element it feeds and
   CONTAINED there: the sets below are asserted exactly, "non-finite" = Inf or NaN, "untouched" = the bits of the clean run. Then the
   parameter-gradient outputs of one case per brick go to mdr_optim_step as the g of a small table: the step is skipped, the scale halves,
   p, m, v and p16 keep their bits and g is all +0.
B  a FINITE input whose result leaves fp16 becomes +-Inf of the right sign: every live element of an fp16 output is classified from the fp64
   reference and the brick's own derived bound (overflow_ref.classify) and must be what its class says; no tolerance is added. The Linear's dX,
   the LayerNorm's dx16, the attention's dQ | dK | dV in both modes, and the O1 loss's gradients (fp32 sums of fp16-rounded terms).

The attention backward's part A is tests/test_attention_grad_gpu.py::test_non_finite_gradients_stay_in_their_sequence.
"""
import time

import numpy as np
import pytest

import embedding_grad_ref as eref
import layernorm_grad_ref as nref
import linear_grad_ref as lref
import mhop_loss_ref
import overflow_ref as ov
import gemm_ref
import test_attention_grad_gpu as at
import test_embedding_grad_gpu as et
import test_gemm_exact_gpu as gt
import test_inbatch_grad_gpu as it
import test_layernorm_grad_gpu as nt
import test_linear_grad_gpu as lt
import test_optim_gpu as ot
from oracle import fp, seeded
from oracle.fp import bits, same_bits

pytestmark = pytest.mark.gpu

PLANTS = [pytest.param(np.inf, id="+inf"), pytest.param(-np.inf, id="-inf"), pytest.param(np.nan, id="nan")]
TINY = seeded.TINY


def bad(a):
    """bool array: the non-finite elements"""
    return ~np.isfinite(np.asarray(a).astype(np.float32))


def planted(a, at, v):
    out = a.copy()
    out[at] = v
    return out


def rows_but(n, i):
    return np.arange(n) != i


# ---- delivery: a brick's parameter gradients as the g of an optimizer table ------------------------------------------------------------------
def assert_delivered(grads, label):
    """grads: float32 arrays, at least one with a non-finite element. One mdr_optim_step over a table whose g they are."""
    grads = [np.ascontiguousarray(g, dtype=np.float32).reshape(-1) for g in grads]
    assert any(bad(g).any() for g in grads), (label, "nothing non-finite to deliver")
    t = ot.Table([g.size for g in grads], 5, 0.0)
    before = t.read()
    t.set_grads(grads)
    t.step()
    st = t.read_state()
    assert st["skipped_last"] == 1 and st["skipped_total"] == 1 and st["adam_step"] == 0, (label, st)
    assert st["loss_scale"] == np.float32(2.0 ** 15), (label, st["loss_scale"])
    after = t.read()
    for name, a, b in zip("p m v p16".split(), before[:4], after[:4]):
        for x, y in zip(a, b):
            assert (x is None and y is None) or same_bits(x, y), (label, name, "a skipped step changed it")
    for g, n in zip(after[4], t.sizes):
        assert not bits(g[:n]).any(), (label, "g is not all +0 after the skipped step")


# ---- A: the Linear ---------------------------------------------------------------------------------------------------------------------------
def linear_inputs(M, N, K, gelu):
    x, w, dy = lref.realistic(M, N, K, 43)
    pre = lt.forward_hook(x, w, lref.bias(N, 43), 0) if gelu else None
    return x, w, dy, pre


def assert_dy_sets(got, clean, rows, m0, n0, label):
    assert bad(got["dx"][m0]).all(), (label, "dx row")
    assert same_bits(got["dx"][:rows][rows_but(rows, m0)], clean["dx"][:rows][rows_but(rows, m0)]), (label, "other dx rows")
    N = got["db"].shape[0]
    assert bad(got["dw"][n0]).all() and same_bits(got["dw"][rows_but(N, n0)], clean["dw"][rows_but(N, n0)]), (label, "dw")
    assert bad(got["db"][n0]) and same_bits(got["db"][rows_but(N, n0)], clean["db"][rows_but(N, n0)]), (label, "db")


@pytest.mark.parametrize("v", PLANTS)
@pytest.mark.parametrize("gelu", [False, True], ids=["identity", "gelu"])
@pytest.mark.parametrize("M,rows,N,K", ov.LINEAR_SHAPES, ids=lambda s: str(s))
def test_a_linear_delivers_and_contains(M, rows, N, K, gelu, v):
    t0 = time.time()
    x, w, dy, pre = linear_inputs(M, N, K, gelu)
    clean = lt.run(x, w, dy, pre, m=rows)
    assert not any(bad(clean[k][:rows] if k == "dx" else clean[k]).any() for k in clean)
    n0, k0 = N - 3, 5
    last = (rows - 1) // lref.SLAB * lref.SLAB + 1      # a row of the last, partial slab
    assert rows % lref.SLAB and last < rows and last >= lref.SLAB
    for m0 in (3, last):
        got = lt.run(x, w, planted(dy, (m0, n0), v), pre, m=rows)
        assert_dy_sets(got, clean, rows, m0, n0, f"dy[{m0}, {n0}] = {v}")
        if gelu:
            got = lt.run(x, w, dy, planted(pre, (m0, n0), v), m=rows)
            assert_dy_sets(got, clean, rows, m0, n0, f"pre[{m0}, {n0}] = {v}")
        # x: the column k0 of dW wherever dZ[m0, n] is not zero; nothing else
        got = lt.run(planted(x, (m0, k0), v), w, dy, pre, m=rows)
        dz = lref.reference_and_bound(x, w, dy, pre, rows)["dz"][0]
        assert (dz[m0] != 0).any() and bad(got["dw"][dz[m0] != 0, k0]).all(), ("x", m0)
        assert same_bits(got["dw"][:, rows_but(K, k0)], clean["dw"][:, rows_but(K, k0)]) and same_bits(got["db"], clean["db"]), ("x", m0)
        assert same_bits(got["dx"][:rows], clean["dx"][:rows]), ("x", m0, "dx")
    # accumulate: finite old values, the same sets
    old_dw, old_db = fp.grid((N, K), 8, 4.0), fp.grid((N,), 9, 4.0)
    clean_acc = lt.run(x, w, dy, pre, m=rows, old_dw=old_dw, old_db=old_db, accumulate=True)
    got = lt.run(x, w, planted(dy, (last, n0), v), pre, m=rows, old_dw=old_dw, old_db=old_db, accumulate=True)
    assert_dy_sets(got, clean_acc, rows, last, n0, f"accumulate dy[{last}, {n0}] = {v}")
    if not gelu and M == 70:
        assert_delivered([got["dw"], got["db"]], "linear")
    print(f"WALL a linear {M} {N} {K} gelu={gelu} {time.time() - t0:.2f} s")


# ---- A: the LayerNorm and the CLS gather -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", PLANTS)
@pytest.mark.parametrize("form", list(ov.LN_FORMS))
@pytest.mark.parametrize("M,rows,H", ov.LN_SHAPES, ids=lambda s: str(s))
def test_a_layernorm_delivers_and_contains(M, rows, H, form, v):
    t0 = time.time()
    case = nref.make_case("unit", ("f32", "res32", True, "f32" if form == "dy16+dy2" else None), M, H, 47)
    assert case["dy16"] is not None and (case["dy2"] is not None) == (form == "dy16+dy2") and case["res"] is not None
    clean = nt.run(**case, m=rows)
    assert not any(bad(clean[k][:rows] if k.startswith("dx") else clean[k]).any() for k in clean)
    c0 = H - 7

    def others_untouched(got, m0, label):
        for k in ("dx16", "dx32"):
            assert bad(got[k][m0]).all(), (label, k, "the row")
            assert same_bits(got[k][:rows][rows_but(rows, m0)], clean[k][:rows][rows_but(rows, m0)]), (label, k, "other rows")

    for m0 in (2, rows - 1):
        for key in ("dy16", "dy2") if case["dy2"] is not None else ("dy16",):
            got = nt.run(**dict(case, **{key: planted(case[key], (m0, c0), v)}), m=rows)
            label = f"{key}[{m0}, {c0}] = {v}"
            others_untouched(got, m0, label)
            for k in ("dg", "db"):
                assert bad(got[k][c0]) and same_bits(got[k][rows_but(H, c0)], clean[k][rows_but(H, c0)]), (label, k)
        dy = case["dy16"].astype(np.float64) + (0 if case["dy2"] is None else case["dy2"].astype(np.float64))
        for key in ("inp", "res"):
            got = nt.run(**dict(case, **{key: planted(case[key], (m0, c0), v)}), m=rows)
            label = f"{key}[{m0}, {c0}] = {v}"
            others_untouched(got, m0, label)
            assert (dy[m0] != 0).any() and bad(got["dg"][dy[m0] != 0]).all(), (label, "dg")
            assert same_bits(got["db"], clean["db"]), (label, "db")
    if H == 64 and form == "dy16":
        got = nt.run(**dict(case, dy16=planted(case["dy16"], (rows - 1, c0), v)), m=rows)
        assert_delivered([got["dg"], got["db"]], "layernorm")
    print(f"WALL a layernorm {M} {H} {form} {time.time() - t0:.2f} s")


@pytest.mark.parametrize("v", PLANTS)
def test_a_gather_cls_backward_lands_on_its_row_only(v):
    import torch
    from multihop_dense_retrieval_amd import layernorm
    H, lens = 64, [5, 1, 64, 7]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T = int(cu[-1])
    dx = fp.grid((T + 3, H), 51, dtype=np.float16)
    d_cls = fp.grid((len(lens), H), 52, dtype=np.float16)
    tcu = torch.from_numpy(cu).cuda()
    clean = layernorm.gather_cls_backward(torch.from_numpy(d_cls).cuda(), tcu, torch.from_numpy(dx).cuda().clone()).cpu().numpy()
    assert not bad(clean).any()
    for b in (0, 2, 3):
        got = layernorm.gather_cls_backward(torch.from_numpy(planted(d_cls, (b, 9), v)).cuda(), tcu, torch.from_numpy(dx).cuda().clone()).cpu().numpy()
        assert bad(got[cu[b], 9])
        hit = np.zeros(got.shape, bool)
        hit[cu[b], 9] = True
        assert np.array_equal(bits(got)[~hit], bits(clean)[~hit]), (b, "something but row cu[b] changed")


# ---- A: the embedding ------------------------------------------------------------------------------------------------------------------------
def embedding_case():
    """TINY's tables; one word row owned by one token, one by 20 (two pieces of 16), the pad row by 3, 40 other rows by one or two"""
    H, vocab, max_pos = TINY["hidden"], TINY["vocab"], TINY["max_pos"]
    counts = {7: 1, 9: 20, TINY["pad_id"]: 3}
    counts.update({100 + 3 * i: 1 + i % 2 for i in range(40)})
    pack = eref.make_flat(counts, 53, vocab=vocab, max_pos=max_pos)
    cap = len(pack["tok_src"])
    return dict(**pack, **eref.make_tables("unit", H, 53, vocab=vocab, max_pos=max_pos), **eref.make_dy("both", cap, H, 53), pad_row=TINY["pad_id"])


@pytest.mark.parametrize("v", PLANTS)
@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_a_embedding_delivers_and_contains(accumulate, v):
    t0 = time.time()
    case = embedding_case()
    H, total = TINY["hidden"], case["total"]
    wid, prow = eref.rows(case)
    old = et.old_values(case, 12) if accumulate else None
    clean = et.run_backward(case, old=old, accumulate=accumulate)
    assert not any(bad(clean[k]).any() for k in clean)
    owners = np.bincount(wid[:total], minlength=TINY["vocab"])
    assert owners[7] == 1 and owners[9] == 20 > eref.P
    c0 = 77
    for wrow in (7, 9):
        t0_ = int(np.flatnonzero(wid[:total] == wrow)[-1])   # (of the 20 owners: the last, in the second piece)
        got = et.run_backward(dict(case, dy16=planted(case["dy16"], (t0_, c0), v)), old=old, accumulate=accumulate)
        label = f"dy16[{t0_}, {c0}] = {v} word row {wrow}"
        assert bad(got["dword"][wrow]).all() and bad(got["dpos"][prow[t0_]]).all() and bad(got["dtype0"]).all(), label
        assert bad(got["dg"][c0]) and bad(got["db"][c0]), label
        for k in ("dg", "db"):
            assert same_bits(got[k][rows_but(H, c0)], clean[k][rows_but(H, c0)]), (label, k)
        assert same_bits(np.delete(got["dword"], wrow, 0), np.delete(clean["dword"], wrow, 0)), (label, "other word rows")
        assert same_bits(np.delete(got["dpos"], prow[t0_], 0), np.delete(clean["dpos"], prow[t0_], 0)), (label, "other position rows")
        assert same_bits(got["d"][rows_but(total, t0_)], clean["d"][rows_but(total, t0_)]) and bad(got["d"][t0_]).all(), (label, "d")
        if not accumulate:
            empty = owners == 0
            empty[TINY["pad_id"]] = True
            assert empty.sum() > 400 and not bits(got["dword"][empty]).any(), (label, "a row that owns no token, or the pad row, is not +0")
            pos_empty = np.bincount(prow[:total], minlength=TINY["max_pos"]) == 0
            assert not bits(got["dpos"][pos_empty]).any(), label
    if not accumulate:
        assert_delivered([got[k] for k in ("dword", "dpos", "dtype0", "dg", "db")], "embedding")
    print(f"WALL a embedding accumulate={accumulate} {time.time() - t0:.2f} s")


# ---- A: the in-batch loss --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", PLANTS)
@pytest.mark.parametrize("mode", [it.F32, it.O1], ids=["f32", "o1"])
@pytest.mark.parametrize("B,d,K", [(1, 32, 0), (17, 768, 17), (33, 768, 1)])
def test_a_inbatch_loss_delivers_and_contains(B, d, K, mode, v):
    """include/mdr_inbatch_loss.h: a row whose lse is NaN has NaN gradients in its own dq / dqsp / dneg rows and in every dctx row it
    contributes to. A NaN element of q[i0] makes every score of hop 1's row i0 NaN, its lse NaN and the loss NaN. Hop 1's row i0 contributes to
    every context column but the one it masks, c2[i0]: that row meets the planted element only through 0 * x (one element) and is left out of
    both sets. Hop 2 never sees q; a NaN element of q_sp1[i0] likewise, hop 2 masking nothing.
    An Inf element makes the scores of row i0 +Inf and -Inf by the sign of the column's element. IEEE rules then give lse = +Inf where a +Inf
    score exists, p = exp(-Inf - Inf) = 0 at a -Inf score and exp(Inf - Inf) = NaN at a +Inf one: the header promises nothing for such a row
    beyond IEEE propagation, and what IEEE propagation gives whatever the signs are is asserted: a non-finite loss, every element of the row's
    own dq non-finite (some score is +Inf, or all are -Inf and lse is NaN), column `col` of every context row the hop feeds non-finite (the
    product of that row's g with the Inf element), and everything the row does not feed untouched."""
    t0 = time.time()
    inp, queue = mhop_loss_ref.make_inputs(B, d, K, seed=7 * B + d + K)
    g0 = 1.0 if mode == it.F32 else it.O1_SCALE
    _, clean = it.run(inp, queue, mode, g0)
    assert not any(bad(clean[k]).any() for k in clean)
    i0, col = B // 2, d - 3
    for leaf, own, other in (("q", "q", "q_sp1"), ("q_sp1", "q_sp1", "q")):
        loss, got = it.run(dict(inp, **{leaf: planted(inp[leaf], (i0, col), v)}), queue, mode, g0)
        label = f"{leaf}[{i0}, {col}] = {v}"
        assert np.isnan(loss) if np.isnan(v) else not np.isfinite(loss), label
        assert bad(got[own][i0]).all() and same_bits(got[own][rows_but(B, i0)], clean[own][rows_but(B, i0)]), (label, "its own row of d" + own)
        assert same_bits(got[other], clean[other]), (label, "the other hop's queries")
        for k in ("neg_1", "neg_2"):
            assert same_bits(got[k][rows_but(B, i0)], clean[k][rows_but(B, i0)]), (label, k, "another row's negatives")
        # every context row the hop feeds gets g * x[i0, col] at column `col`: g * Inf is Inf, or NaN where g is 0 or NaN -- non-finite whatever v is
        keep = rows_but(B, i0) if leaf == "q" else np.ones(B, bool)
        assert bad(got["c1"][:, col]).all() and bad(got["c2"][keep, col]).all(), (label, "column `col` of the context gradients")
        if np.isnan(v):
            assert bad(got["neg_1"][i0]).all() and bad(got["neg_2"][i0]).all() and bad(got["c1"]).all() and bad(got["c2"][keep]).all(), label
    print(f"WALL a inbatch {B} {d} {K} mode={mode} {time.time() - t0:.2f} s")


def test_a_inbatch_loss_reaches_the_flag_through_the_head():
    """the loss's gradient is no parameter's: it reaches one through project.1, the LayerNorm whose input gradient it is"""
    B, d = 17, 768
    inp, queue = mhop_loss_ref.make_inputs(B, d, 17, seed=7 * B + d + 17)
    _, got = it.run(dict(inp, q=planted(inp["q"], (3, 5), np.inf)), queue, it.O1, it.O1_SCALE)
    case = nref.make_case("unit", ("f32", "none", None, "f32"), B, d, 59)
    out = nt.run(**dict(case, dy2=got["q"].astype(np.float32)))
    assert bad(out["db"]).all() and bad(out["dg"]).all()
    assert_delivered([out["dg"], out["db"]], "loss -> project.1")


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,rows,N,K,gelu", ov.LINEAR_CASES)
def test_b_linear_dx_leaves_fp16_as_inf_of_the_right_sign(M, rows, N, K, gelu):
    t0 = time.time()
    c = ov.linear_case(M, rows, N, K, gelu)
    got = lt.run(c["x"], c["w"], c["dy"], c["pre"], m=rows)
    r, b = c["ref"]["dx"]
    fails = ov.verdicts(got["dx"][:rows], r, b, c["cls"], "dx")
    sh = ov.shares(c["cls"])
    print(f"B linear M={M} N={N} K={K} gelu={gelu} s_dy={c['s_dy']:g} s_w={c['s_w']:g} classes {sh}")
    # dW and db are fp32: inside the bound, except where an overflowed dZ feeds them, and there non-finite -- the overflow is delivered
    dz, edz = c["ref"]["dz"]
    over = (np.abs(dz) - edz >= fp.F16_EDGE).any(axis=0)
    doubt = (np.abs(dz) + edz >= fp.F16_EDGE).any(axis=0) & ~over
    assert over.any() == gelu
    fine = ~over & ~doubt
    for name in ("dw", "db"):
        g = got[name]
        if over.any() and not bad(g[over]).all():
            fails.append(f"{name}: an overflowed dZ did not reach it")
        worst, at = fp.worst_ratio(g[fine], c["ref"][name][0][fine], c["ref"][name][1][fine])
        print(f"B linear {name} worst |err| / bound {worst:.4f}")
        if not worst <= 1.0:
            fails.append(f"{name} outside the bound: {worst:.3f} at {at}")
    assert not fails, fails
    print(f"WALL b linear {M} {N} {K} gelu={gelu} {time.time() - t0:.2f} s")


@pytest.mark.parametrize("form", list(ov.LN_FORMS))
@pytest.mark.parametrize("M,rows,H", ov.LN_SHAPES, ids=lambda s: str(s))
def test_b_layernorm_dx16_leaves_fp16_as_inf_of_the_right_sign(M, rows, H, form):
    t0 = time.time()
    c = ov.layernorm_case(M, rows, H, form)
    got = nt.run(**c["args"], m=rows)
    r, b = c["ref"]["dx"]
    fails = ov.verdicts(got["dx16"][:rows], r, b, c["cls"], "dx16", final_rounding_in_b=False)
    print(f"B layernorm M={M} H={H} {form} s={c['s']:g} classes {ov.shares(c['cls'])}")
    err32 = np.abs(got["dx32"][:rows].astype(np.float64) - r)
    if not (err32 <= b).all():   # the fp32 copy of the same value does not overflow
        fails.append(f"dx32 outside the bound at {np.argwhere(~(err32 <= b))[0]}")
    for name in ("dg", "db"):
        worst, at = fp.worst_ratio(got[name], *c["ref"][name])
        if not worst <= 1.0:
            fails.append(f"{name} outside the bound: {worst:.3f} at {at}")
    assert not fails, fails
    print(f"WALL b layernorm {M} {H} {form} {time.time() - t0:.2f} s")


@pytest.mark.parametrize("mode", [0, 3])
def test_b_attention_dqkv_leaves_fp16_as_inf_of_the_right_sign(mode):
    """dQ | dK | dV of one call, every element (overflow_ref.attention_case): FINITE inside attention_grad_ref's bound, INF where the fp32 sum
    leaves fp16 though no dS16 that feeds it does, non-finite where an overflowed dS16 feeds it. A saturating store, or a dS16 conversion that
    clamps, fails the INF or the POISON class."""
    t0 = time.time()
    c = ov.attention_case(mode)
    got = at.run(c["qkv"], c["dctx"], c["cu"], c["heads"], c["L"], mode)
    hidden = 64 * c["heads"]
    print(f"B attention mode={mode} (a, v, e)={ov.ATTN_POWERS[mode]} classes {ov.shares(c['cls'][c['live']])}")
    for i, n in enumerate(("dQ", "dK", "dV")):
        g = got[:, i * hidden:(i + 1) * hidden].astype(np.float32)
        print(f"B attention {n}: {int(np.isinf(g).sum())} Inf, {int(np.isnan(g).sum())} NaN of {g.size}")
    fails = ov.verdicts(got, *c["ref"], c["cls"], "dQ | dK | dV")
    assert not fails, fails
    print(f"WALL b attention mode={mode} {time.time() - t0:.2f} s")


def test_b_the_o1_loss_gradients_are_what_their_rounding_points_say():
    """the six fp32 gradients of one O1 call, every element (overflow_ref.loss_case): each is a sum of fp16-rounded terms, so it is inside
    mhop_loss_ref's O1 bound where nothing that feeds it can overflow, Inf of the term's sign where a term does, non-finite where a g does"""
    t0 = time.time()
    c = ov.loss_case()
    loss, got = it.run(c["inp"], c["queue"], it.O1, c["g0"])
    ref = mhop_loss_ref.loss_and_grads(c["inp"], c["queue"], g0=c["g0"], o1=True)
    assert abs(float(loss) - ref["loss"]) <= ref["loss_bound"], "the forward does not see g0"
    fails = []
    for k in mhop_loss_ref.KEYS:
        g = np.asarray(got[k])
        print(f"B loss {k}: classes {ov.shares(c['cls'][k])}; {int(np.isinf(g).sum())} Inf, {int(np.isnan(g).sum())} NaN of {g.size}")
        fails += ov.verdicts(g, *c["ref"][k], c["cls"][k], k)
    assert not fails, fails
    print(f"WALL b loss {time.time() - t0:.2f} s")


@pytest.mark.parametrize("kernel", gemm_ref.KERNELS)
def test_b_every_gemm_epilogue_overflows_to_inf_bit_for_bit(kernel):
    """dX = dZ W IS the encoder's forward GEMM with an fp16 epilogue, and launch_gemm picks one of six kernels by the problem size: the shapes
    above reach the one-tile kernels only, the persistent 256x128 and 256x256 ones pack their halves through a helper of their own. Every
    kernel, selected through the test hook, on integers: x multiples of 8 up to 128, w multiples of 1 up to 64, an integer bias, K = 256, so
    that every fp32 partial sum in any order is an integer below 2^24 and exact. The fp16 output must EQUAL the one rounding of the exact
    value, +-Inf from 65520 on: no bound at all."""
    M, N, K = 300, 256, 256
    x = fp.grid((M, K), 61, 64.0, np.float16)
    w = fp.grid((N, K), 62, 32.0, np.float16)
    b = np.round(gemm_ref.grid_bias(N, 63).astype(np.float64) * 64).astype(np.float32)
    X, W = x.astype(np.float64), w.astype(np.float64)
    assert (X == np.round(X)).all() and (W == np.round(W)).all() and (np.abs(X) @ np.abs(W).T + np.abs(b)).max() <= 2.0 ** 24
    z = X @ W.T + b.astype(np.float64)
    with np.errstate(over="ignore"):
        want = z.astype(np.float16)
    cls = ov.classify(z, np.zeros_like(z))
    assert ov.cap_failures(cls) == [], ov.shares(cls)
    fl = gt.flavour_of(kernel, M, N, K, 0)
    assert kernel == 0 or fl == gemm_ref.NOMINAL[kernel], (kernel, fl)   # (the kernel asked for is the kernel that ran)
    got, _ = gt.run(x, w, b, 0, kernel)
    print(f"B gemm kernel {kernel} ({fl}): classes {ov.shares(cls)}")
    assert np.array_equal(bits(got), bits(want)), (kernel, fl, "not the one rounding of the exact value")


def test_b_the_o1_loss_at_b1_overflows_at_2_16_and_not_at_2_12():
    """tests/test_inbatch_grad_gpu.py's docstring, as an assertion: at B = 1 the fp16 g = (p - onehot) g0 and its contractions leave fp16 at
    amp's starting scale 2^16 (the reference regime says so: tests/test_overflow_host.py), and stay inside at 2^12"""
    inp, _ = mhop_loss_ref.make_inputs(1, 32, 0, seed=7 + 32)
    loss_hi, hi = it.run(inp, None, it.O1, 2.0 ** 16)
    loss_lo, lo = it.run(inp, None, it.O1, 2.0 ** 12)
    assert np.isfinite(loss_hi) and np.isfinite(loss_lo)
    assert any(bad(hi[k]).any() for k in hi), "2^16 at B = 1 did not overflow"
    assert not any(bad(lo[k]).any() for k in lo), "2^12 at B = 1 overflowed"
