"""CPU (-m "not gpu"): oracle/trunk_rows_oracle.py is checked before tests/test_trunk_rows_gpu.py trusts it.

1. It agrees with independent statements: torch.nn.functional.layer_norm in fp64, oracle/roberta_oracle.py, a stable np.argsort.
2. Its bound holds a SECOND correct fp32 implementation (`model_ln`: pairwise sums where the kernel sums per lane and then over a butterfly; 1 / sqrt
   where the kernel has rsqrtf) on every input family, and that implementation's fp16 rounding passes the fp16 rule.
3. Each wrong formula is thrown out by the same assertions (assert_f32 / assert_f16 / assert_pack / assert_f16_conversion) on the same families.
"""
import numpy as np
import pytest

from guarded import ISENTINEL
from oracle import roberta_oracle
from oracle import trunk_rows_oracle as tr

HS = (128, 256, 384, 1024)  # the scalar path and the 16-byte path, smallest and largest
f32 = np.float32


def psum(a):
    """fp32 pairwise sum over the last axis (neighbours first), [..., 1]."""
    a = np.asarray(a, f32)
    while a.shape[-1] > 1:
        n = a.shape[-1]
        head = a[..., 0:n - n % 2:2] + a[..., 1:n:2]
        a = np.concatenate([head, a[..., n - 1:]], -1) if n % 2 else head
    return a


def model_ln(x, g, b, eps, defect=None):
    """fp32 LayerNorm of fp32 rows x, every operation rounded to fp32. -> (y fp32, y rounded to fp16). `defect`: one of the wrong formulas."""
    x = np.asarray(x, f32)
    H = x.shape[-1]
    g, b, eps = np.asarray(g, f32), np.asarray(b, f32), f32(eps)
    if defect == "swap_gamma_beta":
        g, b = b, g
    if defect == "lost_lane_step":
        k = 64 * (H // 64) - 64
        mu = psum(x[..., :k]) / f32(H)
    else:
        mu = psum(x) / f32(H)
    d = x - mu
    if defect == "one_pass_var":
        var = psum(x * x) / f32(H) - mu * mu
    elif defect == "var_h_minus_1":
        var = psum(d * d) / f32(H - 1)
    else:
        var = psum(d * d) / f32(H)
    if defect == "eps_dropped":
        r = f32(1) / np.sqrt(var)
    elif defect == "eps_outside_root":
        r = f32(1) / (np.sqrt(var) + eps)
    else:
        r = f32(1) / np.sqrt(var + eps)
    t = d * r
    if defect == "fp16_before_affine":
        t = t.astype(np.float16).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (t * g + b).astype(f32)
        return y, y.astype(np.float16)


def model_x(case, defect=None):
    """The kernel's fp32 x = in + residual (one rounded add)."""
    inp, res = case["inp"].astype(f32), case["res"]
    if res is None or defect == "residual_missing":
        return inp
    if defect == "res16_for_res32" and res.dtype == np.float32:
        res = res.astype(np.float16)
    x = inp + res.astype(f32)
    return x + res.astype(f32) if defect == "residual_twice" else x


def ln_cases(rows=5):
    for fam, (_, types, epss) in tr.LN_FAMILIES.items():
        for in_type in types:
            for residual in ("none", "res16", "res32"):
                for H in HS:
                    for eps in epss:
                        yield fam, in_type, residual, H, eps, tr.ln_case(fam, in_type, residual, rows, H, 3)


def check_ln(case, eps, y32, y16, label):
    x, dx = tr.ln_inputs(case["inp"], case["res"])
    ref, bnd = tr.layer_norm(x, case["g"], case["b"], eps), tr.bound(x, dx, case["g"], case["b"], eps)
    return tr.assert_f32(y32, ref, bnd, label), tr.assert_f16(y16, ref, bnd, label)


def test_layer_norm_agrees_with_torch_fp64_and_the_encoder_oracle():
    import torch
    for fam, in_type, residual, H, eps, case in ln_cases():
        x, _ = tr.ln_inputs(case["inp"], case["res"])
        ref = tr.layer_norm(x, case["g"], case["b"], eps)
        t = torch.nn.functional.layer_norm(torch.from_numpy(x), (H,), torch.from_numpy(case["g"].astype(np.float64)), torch.from_numpy(case["b"].astype(np.float64)), eps)
        scale = np.abs(ref).max() + 1.0
        assert np.abs(ref - t.numpy()).max() <= 1e-9 * scale * (1 + np.abs(x).max()), (fam, H)
        other = roberta_oracle.layer_norm(x, case["g"].astype(np.float64), case["b"].astype(np.float64), eps)
        assert np.abs(ref - other).max() <= 1e-9 * scale * (1 + np.abs(x).max()), (fam, H)


def test_packing_agrees_with_independent_statements():
    for B, L, kind, mask_kind, pad_id in tr.PACK_CASES:
        if B * L > 70000:
            continue
        ids, mask = tr.make_pack_case(kind, B, L, pad_id, 1, mask_kind)
        assert np.array_equal(tr.position_ids_full(ids, pad_id), tr.position_ids_loop(ids, pad_id))
        assert np.array_equal(tr.position_ids_full(ids, pad_id), roberta_oracle.position_ids(ids, pad_id))
        n = tr.lens(mask)
        assert np.array_equal(tr.order(mask), np.argsort(-n.astype(np.int64), kind="stable"))
        assert np.array_equal(n, np.asarray([np.count_nonzero(r) for r in mask]))
        got = tr.pack(ids, mask, pad_id)
        assert got["cu"][0] == 0 and np.array_equal(np.diff(got["cu"]), n) and got["total"][0] == n.sum()
        assert np.array_equal(got["tok_src"], np.asarray([b * L + p for b in range(B) for p in range(L) if mask[b, p] != 0], np.int32).reshape(-1))
    # right-padded rows: the sampled ids are the first len entries of roberta_oracle's
    ids, mask = tr.make_pack_case("random", 9, 40, 1, 2)
    full = roberta_oracle.position_ids(ids, 1)
    assert np.array_equal(tr.tok_pid(ids, mask, 1), np.concatenate([full[b, :n] for b, n in enumerate(tr.lens(mask))]))


def test_bound_holds_a_second_implementation_on_every_family():
    """Largest share of `bound` the pairwise fp32 implementation uses, per family (rows = 5, H in 128 / 256 / 384 / 1024, all residual kinds):
    unit 0.40, small_1e-3 0.68, mean100 0.13, mean1000 0.10, outlier60 0.30, const2 0 (exact), gamma_zero_neg 0.21, beta100 0.64, f16_max 0.45,
    f16_subnormal 0.70; the embeddings (test_roberta_embedding_rows_and_offset_table) 0.19, and 0.15 with the offset table. This test prints them
    (SHARES). The bound is worst-case in the direction of every rounding; a correct implementation's roundings mostly
    cancel, so shares of a few per cent up to a third are what a bound that is not slack by orders of magnitude looks like."""
    worst = {}
    for fam, in_type, residual, H, eps, case in ln_cases():
        y32, y16 = model_ln(model_x(case), case["g"], case["b"], eps)
        share, _ = check_ln(case, eps, y32, y16, f"{fam} {in_type} {residual} H={H} eps={eps}")
        worst[fam] = max(worst.get(fam, 0.0), share)
        if fam == "const2":  # the deviations are exactly zero: the output IS beta
            assert np.array_equal(y32, np.broadcast_to(case["b"], y32.shape))
    print("SHARES", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) > 0.02, "the bound is slack by orders of magnitude"


LN_DEFECTS = ["one_pass_var", "var_h_minus_1", "eps_dropped", "eps_outside_root", "residual_missing", "residual_twice", "res16_for_res32", "swap_gamma_beta",
              "fp16_before_affine", "lost_lane_step"]


@pytest.mark.parametrize("defect", LN_DEFECTS)
def test_each_wrong_layernorm_is_rejected(defect):
    rejected = []
    for fam, in_type, residual, H, eps, case in ln_cases():
        with np.errstate(all="ignore"):
            y32, y16 = model_ln(model_x(case, defect), case["g"], case["b"], eps, defect)
        try:
            check_ln(case, eps, y32, y16, defect)
        except AssertionError:
            rejected.append((fam, in_type, residual, H, eps))
    print(defect, "rejected by", len(rejected), "cases, families", sorted({r[0] for r in rejected}))
    assert rejected, f"no family rejects {defect}: a family is missing"
    # and by BOTH output types somewhere: the fp16 rule alone sees it too
    seen16 = False
    for fam, in_type, residual, H, eps, case in ln_cases():
        with np.errstate(all="ignore"):
            _, y16 = model_ln(model_x(case, defect), case["g"], case["b"], eps, defect)
        x, dx = tr.ln_inputs(case["inp"], case["res"])
        try:
            tr.assert_f16(y16, tr.layer_norm(x, case["g"], case["b"], eps), tr.bound(x, dx, case["g"], case["b"], eps))
        except AssertionError:
            seen16 = True
            break
    assert seen16, f"the fp16 rule never rejects {defect}"


# ---- embeddings ----------------------------------------------------------------------------------------------------------------------------
def embed_tables(H, vocab, max_pos, type_rows, seed, pos_offset=0.0):
    rng = np.random.default_rng([seed, H, vocab, max_pos])
    g = (1.0 + 0.3 * rng.standard_normal(H)).astype(f32)
    b = (0.2 * rng.standard_normal(H)).astype(f32)
    return (rng.standard_normal((vocab, H)).astype(f32), (rng.standard_normal((max_pos, H)) + pos_offset).astype(f32),
            rng.standard_normal((type_rows, H)).astype(f32), g, b)


def model_embed(word, pos, typ, wid, prow, trow, g, b, eps):
    x = (word[wid] + pos[prow]) + typ[trow]
    return model_ln(x, g, b, eps)


@pytest.mark.parametrize("defect", [None, "reader_pos_packed_index", "type_row_0"])
def test_reader_embedding_rows(defect):
    H, L, B = 128, 64, 4
    word, pos, typ, g, b = embed_tables(H, 50, L, 2, 5)
    ids, mask = tr.make_pack_case("random", B, L, 0, 4)
    ty = np.random.default_rng(1).integers(-1, 4, (B, L))
    src = tr.tok_src(mask)
    wid, prow, trow = tr.embed_rows(ids.reshape(-1), src, None, word, pos, typ, ty, reader_L=L)
    x, dx = tr.embed_inputs(word, pos, typ, wid, prow, trow)
    ref, bnd = tr.layer_norm(x, g, b, 1e-12), tr.bound(x, dx, g, b, 1e-12)
    if defect == "reader_pos_packed_index":
        prow = np.minimum(np.arange(len(src)), L - 1)
    if defect == "type_row_0":
        trow = np.zeros_like(trow)
    y32, y16 = model_embed(word, pos, typ, wid, prow, trow, g, b, 1e-12)
    if defect is None:
        tr.assert_f32(y32, ref, bnd)
        tr.assert_f16(y16, ref, bnd)
    else:
        with pytest.raises(AssertionError):
            tr.assert_f32(y32, ref, bnd)
        with pytest.raises(AssertionError):
            tr.assert_f16(y16, ref, bnd)


def test_roberta_embedding_rows_and_offset_table():
    for off in (0.0, 30.0):
        H, L, B = 384, 65, 5
        word, pos, typ, g, b = embed_tables(H, 50, 40, 1, 6, off)  # max_pos 40 < L: pid reaches the clamp
        ids, mask = tr.make_pack_case("random", B, L, 1, 4, "holes")
        ids[0, :3] = [-5, 2 ** 31 + 7, 10 ** 12]
        p = tr.pack(ids, mask, 1)
        wid, prow, trow = tr.embed_rows(ids.reshape(-1), p["tok_src"], p["tok_pid"], word, pos, typ)
        assert prow.max() == 39 and wid.max() == 49 and (p["tok_pid"] == 1).any()
        x, dx = tr.embed_inputs(word, pos, typ, wid, prow, trow)
        ref, bnd = tr.layer_norm(x, g, b, 1e-5), tr.bound(x, dx, g, b, 1e-5)
        y32, y16 = model_embed(word, pos, typ, wid, prow, trow, g, b, 1e-5)
        print("embed offset", off, "share", tr.assert_f32(y32, ref, bnd), "neighbours", tr.assert_f16(y16, ref, bnd))


# ---- packing defects -----------------------------------------------------------------------------------------------------------------------
def wrong_pack(ids, mask, pad_id, defect):
    out = tr.pack(ids, mask, pad_id)
    notpad, m = ids != pad_id, mask != 0
    n = out["lens"].astype(np.int64)
    src = out["tok_src"]
    if defect == "pid_without_pad_id":
        out["tok_pid"] = (out["tok_pid"] - pad_id).astype(np.int32)
    elif defect == "pid_from_mask":
        out["tok_pid"] = np.where(m, np.cumsum(m, 1) + pad_id, pad_id).reshape(-1)[src].astype(np.int32)
    elif defect == "pid_exclusive":
        out["tok_pid"] = np.where(notpad, np.cumsum(notpad, 1) - 1 + pad_id, pad_id).reshape(-1)[src].astype(np.int32)
    elif defect == "pid_pad_counted":
        out["tok_pid"] = (np.cumsum(notpad, 1) + pad_id).reshape(-1)[src].astype(np.int32)
    elif defect == "order_ties_high_index":
        out["order"] = np.asarray(sorted(range(len(n)), key=lambda i: (-n[i], -i)), np.int32)
    elif defect == "order_ascending":
        out["order"] = np.argsort(n, kind="stable").astype(np.int32)
    elif defect == "cu_carry_dropped":
        c = np.concatenate([[0], np.cumsum(n[:1024])])
        if len(n) > 1024:
            c = np.concatenate([c[:1024], np.concatenate([[0], np.cumsum(n[1024:])])])
        out["cu"] = c.astype(np.int32)
    else:
        raise ValueError(defect)
    return out


def as_buffers(p, B, L):
    """What the hook's buffers would hold: order untouched above 1024 rows, tok_* untouched beyond total."""
    pad = lambda a: np.concatenate([a, np.full(B * L - len(a), ISENTINEL, np.int32)])  # noqa: E731
    return dict(lens=p["lens"], cu=p["cu"], total=p["total"], order=p["order"] if B <= 1024 else np.full(B, ISENTINEL, np.int32),
                tok_src=pad(p["tok_src"]), tok_pid=pad(p["tok_pid"]))


@pytest.mark.parametrize("defect", [None, "pid_without_pad_id", "pid_from_mask", "pid_exclusive", "pid_pad_counted", "order_ties_high_index", "order_ascending",
                                    "cu_carry_dropped"])
def test_each_wrong_packing_is_rejected(defect):
    rejected = 0
    for B, L, kind, mask_kind, pad_id in tr.PACK_CASES:
        if B * L > 140000:
            continue
        ids, mask = tr.make_pack_case(kind, B, L, pad_id, 1, mask_kind)
        p = tr.pack(ids, mask, pad_id) if defect is None else wrong_pack(ids, mask, pad_id, defect)
        try:
            tr.assert_pack(as_buffers(p, B, L), ids, mask, pad_id, ISENTINEL, f"B={B} L={L} {kind} {mask_kind}")
        except AssertionError:
            rejected += 1
    assert (rejected == 0) if defect is None else rejected > 0, (defect, rejected)


def test_pack_cases_cover_what_they_claim():
    Bs, Ls = {c[0] for c in tr.PACK_CASES}, {c[1] for c in tr.PACK_CASES}
    assert Bs == {1, 3, 4, 5, 63, 64, 65, 1000, 1023, 1024, 1025, 2049, 3000} and Ls == {1, 63, 64, 65, 128, 129, 512}
    ids, mask = tr.make_pack_case("zeros", 1024, 65, 1, 1)
    n = tr.lens(mask)
    assert n[0] == 0 and n[-1] == 0 and n[1023] == 0
    assert ((ids == 1) & (mask != 0)).any()                                    # pad ids masked in
    ids, mask = tr.make_pack_case("random", 64, 129, 0, 1, "holes")
    first = np.argmax(mask != 0, 1)
    assert any(((ids[b, :first[b]] != 0).any() for b in range(64)))           # non-pad ids masked out in front of masked-in ones
    assert np.all(np.diff(tr.lens(tr.make_pack_case("decreasing", 63, 128, 1, 1)[1])) < 0)
    assert np.all(np.diff(tr.lens(tr.make_pack_case("increasing", 64, 129, 0, 1)[1])) > 0)
    assert set(np.unique(tr.make_pack_case("random", 65, 512, 1, 1, "values")[1])) == {-1, 0, 1, 2}


def test_f16_conversion_values_reject_truncation():
    v = tr.f16_conversion_values()
    with np.errstate(over="ignore"):
        tr.assert_f16_conversion(v.astype(np.float16), v)
    # truncation: clear the 13 low mantissa bits of the fp32 value, then convert (exact for normal results)
    trunc = (v.view(np.uint32) & np.uint32(0xFFFFE000)).view(f32)
    with np.errstate(over="ignore"), pytest.raises(AssertionError):
        tr.assert_f16_conversion(trunc.astype(np.float16), v)
    k = np.arange(1024)
    ties = (1.0 + (k + 0.5) * 2.0 ** -10).astype(f32)
    r = ties.astype(np.float16).view(np.uint16)
    assert np.array_equal(r & 1, np.zeros(1024, np.uint16)) and set((r >> 1) & 1) == {0, 1}  # ties go to even, from lower neighbours of both parities
