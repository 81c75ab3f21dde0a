"""GPU (-m gpu): the trunk's packing, embedding, LayerNorm and row kernels, each in isolation through its test hook (mdr_test_pack,
mdr_test_embed_ln, mdr_test_layernorm, mdr_test_row_copy; include/mdr_hip.h), against oracle/trunk_rows_oracle.py.

EVERY output element is compared; nothing is sampled or averaged. Integer outputs must be equal; fp32 outputs must lie inside the oracle's
derived `bound`; fp16 outputs must be RNE16 of the fp64 result unless the bound's interval crosses a rounding boundary. The bound, the assertions
and the input families are the ones tests/test_trunk_rows_oracle.py shows (on the host) to hold a second correct implementation and to throw out
each wrong formula; no tolerance here was read off a device. Every output buffer carries GUARD sentinel rows in front of and behind the call's
own, and rows the call must not write (rows >= rows, tokens >= total, `order` above 1024 sequences) start as sentinels: all must keep their bits.
Each check prints `SHARE kernel=... family=... share=...`, the largest part of the bound the device used (profiles/trunk_rows_bound_usage.md).
"""
import numpy as np
import pytest
import torch

import guarded
from guarded import ISENTINEL, dev
from multihop_dense_retrieval_amd._lib import ptr
from oracle import trunk_rows_oracle as tr

pytestmark = pytest.mark.gpu

GUARD = 8
f32 = np.float32


def lib():
    from multihop_dense_retrieval_amd import _lib
    return _lib, _lib.lib()


def guarded_rows(rows, width, dtype, init=None):
    """A device buffer of `rows` rows (of `width`) between GUARD sentinel rows; `init` (numpy, optional) fills the call's own rows."""
    return guarded.Guarded(rows, (width,), dtype, GUARD, GUARD, init)


def untouched(rows, what):
    guarded.assert_untouched(rows, f"{what} were written")


# ---- packing -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,kind,mask_kind,pad_id", tr.PACK_CASES, ids=[f"B{c[0]}-L{c[1]}-{c[2]}-{c[3]}-pad{c[4]}" for c in tr.PACK_CASES])
def test_pack(B, L, kind, mask_kind, pad_id):
    _lib, L_ = lib()
    ids, mask = tr.make_pack_case(kind, B, L, pad_id, 1, mask_kind)
    bufs = {k: guarded_rows(n, 1, torch.int32) for k, n in (("lens", B), ("cu", B + 1), ("total", 1), ("order", B), ("tok_src", B * L), ("tok_pid", B * L))}
    t_ids, t_mask = dev(ids), dev(mask)  # named, so that both stay allocated across the call
    _lib.check(L_.mdr_test_pack(ptr(t_ids), ptr(t_mask), B, L, pad_id,*(ptr(bufs[k].own) for k in ("lens", "cu", "total", "order", "tok_src", "tok_pid")),
                                0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    tr.assert_pack({k: v.checked().reshape(-1) for k, v in bufs.items()}, ids, mask, pad_id, ISENTINEL, f"B={B} L={L} {kind} {mask_kind} pad_id={pad_id}")


# ---- embeddings + LayerNorm ----------------------------------------------------------------------------------------------------------------
def embed_tables(H, vocab, max_pos, type_rows, seed, pos_offset=0.0):
    rng = np.random.default_rng([seed, H, vocab, max_pos])
    g = (1.0 + 0.3 * rng.standard_normal(H)).astype(f32)
    b = (0.2 * rng.standard_normal(H)).astype(f32)
    return (rng.standard_normal((vocab, H)).astype(f32), (rng.standard_normal((max_pos, H)) + pos_offset).astype(f32),
            rng.standard_normal((type_rows, H)).astype(f32), g, b)


def run_embed(flavour, ids, mask, ty, pad_id, tables, eps, with32, L, label, total_override=None):
    """One hook call over the packing the oracle states for (ids, mask). Compares every row < total and demands sentinels behind."""
    _lib, L_ = lib()
    word, pos, typ, g, b = tables
    H, cap = word.shape[1], ids.size
    p = tr.pack(ids, mask, pad_id)
    total = int(p["total"][0]) if total_override is None else total_override
    src, pid = p["tok_src"][:total], p["tok_pid"][:total]
    fill = lambda a: np.concatenate([a, np.zeros(cap - len(a), np.int32)])  # noqa: E731  (entries behind total: valid indices, never to be read)
    out16, out32 = guarded_rows(cap, H, torch.float16), (guarded_rows(cap, H, torch.float32) if with32 else None)
    t_ids, t_ty, t_src, t_pid, t_tot = dev(ids), (dev(ty) if ty is not None else None), dev(fill(p["tok_src"])), dev(fill(p["tok_pid"])), dev(np.asarray([total], np.int32))
    t_tab = [dev(a) for a in (word, pos, typ, g, b)]
    _lib.check(L_.mdr_test_embed_ln(flavour, ptr(t_ids), ptr(t_ty), ptr(t_src), ptr(t_pid), ptr(t_tot), cap, L, ptr(t_tab[0]), ptr(t_tab[1]), ptr(t_tab[2]),
                                    typ.shape[0], ptr(t_tab[3]), ptr(t_tab[4]), H, word.shape[0], pos.shape[0], eps, ptr(out16.own),
                                    ptr(out32.own) if with32 else None, 0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    wid, prow, trow = tr.embed_rows(ids.reshape(-1), src, pid, word, pos, typ, ty, reader_L=L if flavour == 1 else None)
    x, dx = tr.embed_inputs(word, pos, typ, wid, prow, trow)
    ref, bnd = tr.layer_norm(x, g, b, eps), tr.bound(x, dx, g, b, eps)
    got16 = out16.checked()
    untouched(got16[total:], "fp16 rows behind total")
    tr.assert_f16(got16[:total], ref, bnd, label)
    if with32:
        got32 = out32.checked()
        untouched(got32[total:], "fp32 rows behind total")
        print(f"SHARE kernel={'reader_embed_ln' if flavour else 'embed_ln'} family={label.split()[0]} share={tr.assert_f32(got32[:total], ref, bnd, label):.4f}")
    return wid, prow, trow, p


def small_batch(total, L=8):
    ids = np.random.default_rng(total).integers(2, 50, (1, L)).astype(np.int64)
    mask = np.zeros((1, L), np.int64)
    mask[0, :total] = 1
    return ids, mask


@pytest.mark.parametrize("H", [128, 384, 768, 1024])
@pytest.mark.parametrize("with32", [True, False], ids=["out32", "no-out32"])
def test_embed_ln_roberta(H, with32):
    for total in (1, 3, 4, 5):
        ids, mask = small_batch(total)
        run_embed(0, ids, mask, None, 1, embed_tables(H, 50, 20, 1, 7), 1e-5, with32, 8, f"unit total={total} H={H}")
    # a few hundred tokens: holes, pad ids inside the rows (pid == pad_id), ids out of range on both sides and beyond 2^31, max_pos below the longest count
    for pad_id, off in ((1, 0.0), (0, 0.0), (1, 30.0)):
        ids, mask = tr.make_pack_case("random", 5, 65, pad_id, 4, "holes")
        ids[:, :4] = np.asarray([-5, 2 ** 31 + 7, 10 ** 12, 50], np.int64)
        mask[:, :4] = 1
        wid, prow, trow, p = run_embed(0, ids, mask, None, pad_id, embed_tables(H, 50, 40, 1, 8, off), 1e-5, with32, 65,
                                       f"{'offset30' if off else 'unit'} holes pad_id={pad_id} H={H}")
        assert prow.max() == 39 and (p["tok_pid"] >= 40).any() and (p["tok_pid"] == pad_id).any() and wid.min() == 0 and wid.max() == 49
        assert int(p["total"][0]) < ids.size
    ids, mask = tr.make_pack_case("random", 5, 65, 1, 5)
    run_embed(0, ids, mask, None, 1, embed_tables(H, 50, 80, 1, 9), 1e-12, with32, 65, f"unit total-below-packing H={H}", total_override=int(tr.lens(mask).sum()) - 3)


@pytest.mark.parametrize("H,L,B", [(128, 1, 5), (384, 64, 4), (768, 512, 2), (1024, 64, 3), (128, 512, 1)])
@pytest.mark.parametrize("with32", [True, False], ids=["out32", "no-out32"])
def test_embed_ln_reader(H, L, B, with32):
    rng = np.random.default_rng([H, L, B])
    ids, mask = tr.make_pack_case("random", B, L, 0, 6)
    mask[:, 0] = 1
    mask[:, L - 1] = 1  # row starts and ends: src % L == 0 and L - 1
    ids[0, 0] = -3
    ids[-1, L - 1] = 2 ** 33
    ty = rng.integers(-2, 5, (B, L)).astype(np.int64)  # a table of 2 rows: out of range on both sides
    tables = embed_tables(H, 50, max(L, 2), 2, 10)
    run_embed(1, ids, mask, ty, 0, tables, 1e-12, with32, L, f"unit reader types L={L} H={H}")
    run_embed(1, ids, mask, None, 0, tables, 1e-12, with32, L, f"unit reader types=NULL L={L} H={H}")
    run_embed(1, ids, mask, ty, 0, embed_tables(H, 50, max(L, 2), 2, 11, 30.0), 1e-12, with32, L, f"offset30 reader L={L} H={H}")


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------------
OUTS = ("out16", "out32", "both", "alias")   # alias: out32 is res32, in place (residual == res32 only; otherwise the turn goes to "both")
ROWS = (1, 3, 4, 5, 1000)
ROWS_DEV = ("null", "below", "above")


def run_layernorm(family, in_type, residual, H, eps, rows_cap, outs, rows_dev, seed):
    _lib, L_ = lib()
    case = tr.ln_case(family, in_type, residual, rows_cap, H, seed)
    if outs == "alias" and residual != "res32":
        outs = "both"
    rows = {"null": rows_cap, "below": rows_cap // 2, "above": rows_cap}[rows_dev]
    t_rows = None if rows_dev == "null" else dev(np.asarray([rows if rows_dev == "below" else rows_cap + 7], np.int32))
    t_in, t_g, t_b = dev(case["inp"]), dev(case["g"]), dev(case["b"])
    t_res = dev(case["res"]) if case["res"] is not None else None
    out16 = guarded_rows(rows_cap, H, torch.float16) if outs != "out32" else None
    out32 = guarded_rows(rows_cap, H, torch.float32, init=case["res"] if outs == "alias" else None) if outs != "out16" else None
    res16 = t_res if residual == "res16" else None
    res32 = (out32.own if outs == "alias" else t_res) if residual == "res32" else None
    _lib.check(L_.mdr_test_layernorm(ptr(t_in), 1 if in_type == "f16" else 0, ptr(res16), ptr(res32), rows_cap, ptr(t_rows), H, ptr(t_g), ptr(t_b), eps,
                                     ptr(out16.own) if out16 else None, ptr(out32.own) if out32 else None, 0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    label = f"{family} {in_type} {residual} H={H} eps={eps} rows={rows}/{rows_cap} {outs} rows_dev={rows_dev}"
    x, dx = tr.ln_inputs(case["inp"], case["res"])
    ref, bnd = tr.layer_norm(x, case["g"], case["b"], eps)[:rows], tr.bound(x, dx, case["g"], case["b"], eps)[:rows]
    if out16:
        got = out16.checked()
        untouched(got[rows:], "fp16 rows behind rows")
        tr.assert_f16(got[:rows], ref, bnd, label)
        if family == "const2":
            assert np.array_equal(tr.bits16(got[:rows]), tr.bits16(np.broadcast_to(case["b"].astype(np.float16), ref.shape))), label
    if out32:
        got = out32.checked()
        if outs == "alias":
            assert np.array_equal(got[rows:].view(np.uint32), case["res"][rows:].view(np.uint32)), "the residual rows behind rows were written"
        else:
            untouched(got[rows:], "fp32 rows behind rows")
        share = tr.assert_f32(got[:rows], ref, bnd, label) if rows else 0.0
        print(f"SHARE kernel=layernorm_{in_type} family={family} share={share:.4f}")
        if family == "const2":
            assert np.array_equal(got[:rows], np.broadcast_to(case["b"], ref.shape)), label  # the deviations are exactly zero: beta


@pytest.mark.parametrize("residual", ["none", "res16", "res32"])
@pytest.mark.parametrize("in_type", ["f32", "f16"])
@pytest.mark.parametrize("H", [128, 256, 384, 512, 640, 768, 896, 1024])
def test_layernorm(H, in_type, residual):
    """Every (path, input type, residual) pairing at every H; inside, every family of the input type at each of its eps values, while the output set,
    the row count and the rows_dev mode take turns; test_layernorm_every_output_set_row_count_and_rows_dev crosses those three in full."""
    turn = (H // 128 - 1) * 6 + (in_type == "f16") * 3 + ["none", "res16", "res32"].index(residual)
    k = 0
    for family, (_, types, epss) in tr.LN_FAMILIES.items():
        if in_type not in types:
            continue
        for eps in epss:
            n = turn + k
            run_layernorm(family, in_type, residual, H, eps, ROWS[n % 5], OUTS[(n // 5 + n) % 4], ROWS_DEV[(n // 2) % 3], seed=n)
            k += 1


@pytest.mark.parametrize("rows_dev", ROWS_DEV)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("outs", OUTS)
def test_layernorm_every_output_set_row_count_and_rows_dev(outs, rows, rows_dev):
    """The full cross of the three launch-side factors, on both paths and both input types (residual res32, so that `alias` is what it says)."""
    for H, in_type in ((256, "f32"), (384, "f16"), (1024, "f16"), (896, "f32")):
        run_layernorm("unit", in_type, "res32", H, 1e-5, rows, outs, rows_dev, seed=1)


# ---- CLS gather, f32 -> f16 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with32", [True, False], ids=["f32-pair", "f16-only"])
@pytest.mark.parametrize("H", [128, 768])
@pytest.mark.parametrize("B", [1, 3, 1025])
def test_gather_cls(B, H, with32):
    _lib, L_ = lib()
    rng = np.random.default_rng([B, H])
    n = rng.integers(1, 6, B)
    cu = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    T = int(cu[-1])
    h16 = rng.standard_normal((T, H)).astype(np.float16)
    h32 = rng.standard_normal((T, H)).astype(f32)
    out16, out32 = guarded_rows(B, H, torch.float16), (guarded_rows(B, H, torch.float32) if with32 else None)
    t16, t32, tcu = dev(h16), (dev(h32) if with32 else None), dev(cu)
    _lib.check(L_.mdr_test_row_copy(0, ptr(t16), ptr(t32), ptr(tcu), B, H, 0, ptr(out16.own), ptr(out32.own) if with32 else None, 0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(tr.bits16(out16.checked()), tr.bits16(h16[cu[:-1]]))
    if with32:
        assert np.array_equal(out32.checked().view(np.uint32), h32[cu[:-1]].view(np.uint32))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 ** 20 + 3])
def test_f32_to_f16(n):
    _lib, L_ = lib()
    special = tr.f16_conversion_values()
    rng = np.random.default_rng(n)
    rand = (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 12, 4096))).astype(f32)
    pool = np.concatenate([special, rand])
    srcs = [np.resize(pool, n)] if n > 257 else [np.resize(np.roll(pool, -s), n) for s in range(0, len(pool), len(pool) // 48)] + [np.asarray([v], f32) for v in (65520.0, 65519.0, -0.0, np.nan) if n == 1]
    for src in srcs:
        src = np.ascontiguousarray(src, f32)
        out = guarded_rows(1, len(src) + 0, torch.float16)  # one row of n elements between GUARD sentinel rows of the same width
        t = dev(src)
        _lib.check(L_.mdr_test_row_copy(1, None, ptr(t), None, 0, 0, len(src), ptr(out.own), None, 0, _lib.current_stream_ptr()))
        torch.cuda.synchronize()
        tr.assert_f16_conversion(out.checked().reshape(-1), src, f"n={n}")


# ---- hook validation -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_errors_and_launch_nothing():
    _lib, L_ = lib()
    i64 = torch.zeros((4, 8), dtype=torch.int64, device="cuda")
    ints = [guarded_rows(64, 1, torch.int32) for _ in range(6)]
    f = torch.zeros((64, 128), dtype=torch.float32, device="cuda")
    o16, o32 = guarded_rows(32, 128, torch.float16), guarded_rows(32, 128, torch.float32)
    one = torch.ones(1, dtype=torch.int32, device="cuda")
    P = ptr

    def pack(ids=P(i64), mask=P(i64), B=4, L=8, lens=P(ints[0].own), cu=P(ints[1].own), total=P(ints[2].own), order=P(ints[3].own), src=P(ints[4].own), pid=P(ints[5].own)):
        return L_.mdr_test_pack(ids, mask, B, L, 1, lens, cu, total, order, src, pid, 0, None)

    def embed(flavour=0, ids=P(i64), src=P(one), pid=P(one), total=P(one), cap=4, L=8, word=P(f), out16=P(o16.own), H=128, vocab=8, max_pos=8, type_vocab=2):
        return L_.mdr_test_embed_ln(flavour, ids, None, src, pid, total, cap, L, word, P(f), P(f), type_vocab, P(f), P(f), H, vocab, max_pos, 1e-5, out16, P(o32.own), 0, None)

    def ln(inp=P(f), in_f16=0, res16=None, res32=None, rows=4, H=128, g=P(f), out16=P(o16.own), out32=P(o32.own)):
        return L_.mdr_test_layernorm(inp, in_f16, res16, res32, rows, None, H, g, P(f), 1e-5, out16, out32, 0, None)

    def copy(mode=0, s16=P(o16.own), s32=None, cu=P(one), B=1, H=128, n=0, out16=P(o16.own), out32=None):
        return L_.mdr_test_row_copy(mode, s16, s32, cu, B, H, n, out16, out32, 0, None)

    bad = [(pack, dict(ids=None), "NULL"), (pack, dict(mask=None), "NULL"), (pack, dict(order=None), "NULL"), (pack, dict(pid=None), "NULL"), (pack, dict(B=0), "B"),
           (pack, dict(B=-1), "B"), (pack, dict(L=0), "L"), (pack, dict(L=513), "L"),
           (embed, dict(ids=None), "NULL"), (embed, dict(out16=None), "NULL"), (embed, dict(pid=None), "NULL"), (embed, dict(word=None), "NULL"), (embed, dict(H=96), "H"),
           (embed, dict(H=1088), "H"), (embed, dict(H=0), "H"), (embed, dict(cap=0), "cap"), (embed, dict(flavour=2), "flavour"), (embed, dict(flavour=1, L=0), "L"),
           (embed, dict(flavour=1, L=513, max_pos=600), "L"), (embed, dict(flavour=1, L=8, max_pos=4), "L"), (embed, dict(vocab=0), "vocab"),
           (ln, dict(inp=None), "NULL"), (ln, dict(g=None), "NULL"), (ln, dict(out16=None, out32=None), "NULL"), (ln, dict(res16=P(o16.own), res32=P(f)), "at most one"),
           (ln, dict(H=96), "H"), (ln, dict(H=1088), "H"), (ln, dict(rows=0), "rows_cap"), (ln, dict(in_f16=2), "in_f16"),
           (copy, dict(s16=None), "NULL"), (copy, dict(cu=None), "NULL"), (copy, dict(out16=None), "NULL"), (copy, dict(s32=P(f)), "NULL"), (copy, dict(B=0), "B"),
           (copy, dict(H=100), "H"), (copy, dict(mode=2), "mode"), (copy, dict(mode=1, s32=None, n=4), "NULL"), (copy, dict(mode=1, s32=P(f), n=0), "n")]
    for fn, kw, word in bad:
        assert fn(**kw) == -1, (fn.__name__, kw)
        assert word in L_.mdr_last_error().decode(), (fn.__name__, kw, L_.mdr_last_error())
    torch.cuda.synchronize()
    for g_ in ints + [o16, o32]:  # none of the rejected calls launched anything: every output buffer is still all sentinels
        untouched(g_.checked(), "buffers of rejected calls")
    with pytest.raises(_lib.MdrError):
        _lib.check(pack(B=0))
    assert pack() == 0 and ln() == 0  # and the same arguments without the defect are accepted
    torch.cuda.synchronize()
