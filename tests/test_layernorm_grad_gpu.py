"""GPU (-m gpu): the LayerNorm backward in isolation (mdr_layernorm_backward, include/mdr_layernorm_grad.h) against the fp64 statement of
tests/layernorm_grad_ref.py, packed_layer_norm (multihop_dense_retrieval_amd/layernorm.py) on top of it, and the backward of the CLS gather
(mdr_gather_cls_backward). EVERY element of dx16, dx32, dg and db is compared; nothing is averaged.

Two bars. Where the arithmetic is exact the result must be EQUAL: db of a dy on the grid of multiples of 1/8 (any fp32 sum of M <= 2^16 such
values of magnitude at most 4 is exact in any order), zeros from dy = 0 and from g = 0, the CLS rows' sums on the grid. Everywhere else the
bar is layernorm_grad_ref's bound, derived from the formats and the rounding points listed in csrc/mdr_layernorm_grad.hip and shown on the
host (tests/test_layernorm_grad_host.py) to hold a second implementation of the dataflow and to throw out each defect; dx16 by the monotonic
fp16 rule of oracle/trunk_rows_oracle.py. No tolerance here was read off a device. Each bound check prints `SHARE ...`, the largest part of
the bound the device used.

Every output starts as a finite sentinel: dx16 and dx32 with 64 guard rows on both sides, dg and db with 64 guard elements on both sides,
which must keep their bits in every call of this file, as must the rows at or behind the valid count. Shapes: H = 64 and 192 (the generic
path with 1 and 3 elements per lane), 256 and 768 (the 16-byte path with 1 and 3 groups), 1024 (the limit); M = 1 .. 9 around the four waves
of a workgroup and one and two chunks, 300, and for H = 64 two M found by calling chunks() whose chunks hold >= 8 rows, do not divide M
and number >= 3; and layernorm_grad_ref.LARGE_HM, the shipping widths at the smallest training row counts at which a wave walks three rows
with dg and db in registers, the last chunk is ragged and a strand of the reduction adds more than sixteen chunks.
"""
import numpy as np
import pytest
import torch

import layernorm_grad_ref as ref
from guarded import E_INVALID, E_WORKSPACE, SENTINEL, Guarded, dev
from multihop_dense_retrieval_amd._lib import ptr
from oracle import fp
from oracle import trunk_rows_oracle as tr
from oracle.fp import bits

pytestmark = pytest.mark.gpu

GUARD = 64        # rows of dx / elements of dg and db in front of and behind the call's own, which must keep their bits


def ms_for(H):
    return ref.M_SWEEP + (ref.split_ms(H) if H == 64 else [])


def combos_for(M):
    return ref.COMBOS if M in (5, 300) else ref.TRUNK_COMBOS


def raw_call(inp, in_f16, res16, res32, dy16, dy2, dy2_f32, M, m_dev, H, g, eps, dx16, dx32, dg, db, accumulate, ws, ws_bytes):
    from multihop_dense_retrieval_amd import _lib, layernorm
    return layernorm.lib().mdr_layernorm_backward(ptr(inp), in_f16, ptr(res16), ptr(res32), ptr(dy16), ptr(dy2), dy2_f32, M, ptr(m_dev), H, ptr(g), eps,
                                                  ptr(dx16), ptr(dx32), ptr(dg), ptr(db), accumulate, ptr(ws), ws_bytes, 0, _lib.current_stream_ptr())


def run(inp, res, dy16, dy2, g, eps=ref.EPS, m=None, outs="xXgb", old_dg=None, old_db=None, accumulate=False, ws_extra=0):
    """One call on numpy inputs. outs: x = dx16, X = dx32, g = dg, b = db. Outputs start as SENTINEL (dg / db: the old values if given) inside
    guards; returns {"dx16": float16 [M, H], "dx32": float32 [M, H] (rows at or behind m still SENTINEL), "dg", "db": float32 [H]} after
    asserting MDR_OK, that the guards and the rows at or behind m kept their bits and that an output not asked for was not written."""
    from multihop_dense_retrieval_amd import _lib, layernorm
    M, H = inp.shape
    b16, b32 = (Guarded(M, (H,), t, GUARD, GUARD, name=name) for t, name in ((torch.float16, "dx16"), (torch.float32, "dx32")))
    bg, bb = (Guarded(H, (), torch.float32, GUARD, GUARD, None if old is None else old.astype(np.float32), name, "elements")
              for old, name in ((old_dg, "dg"), (old_db, "db")))
    want = (1 if "g" in outs else 0) | (2 if "b" in outs else 0)
    need = int(layernorm.lib().mdr_layernorm_backward_workspace_bytes(M, H, want))
    ws = torch.empty(max(need + ws_extra, 16), dtype=torch.uint8, device="cuda")
    m_dev = None if m is None else torch.tensor([m], dtype=torch.int32, device="cuda")
    res16 = res if res is not None and res.dtype == np.float16 else None
    res32 = res if res is not None and res.dtype == np.float32 else None
    held = [dev(a) for a in (inp, res16, res32, dy16, dy2, g)]  # (held until the synchronise below)
    _lib.check(raw_call(held[0], 1 if inp.dtype == np.float16 else 0, held[1], held[2], held[3], held[4], 1 if dy2 is not None and dy2.dtype == np.float32 else 0,
                        M, m_dev, H, held[5], eps, b16.own if "x" in outs else None, b32.own if "X" in outs else None,
                        bg.own if "g" in outs else None, bb.own if "b" in outs else None, 1 if accumulate else 0, ws, need + ws_extra))
    torch.cuda.synchronize()
    mm = M if m is None else min(max(m, 0), M)
    return {"dx16": b16.checked(valid=mm, asked="x" in outs), "dx32": b32.checked(valid=mm, asked="X" in outs),
            "dg": bg.checked(asked="g" in outs), "db": bb.checked(asked="b" in outs)}


def check_bound(got, rb, m, label):
    """every output inside the bound; prints the largest share of the bound used"""
    r, bnd = rb["dx"]
    odd = tr.assert_f16(got["dx16"][:m], r, bnd, label + " dx16")
    shares = {"dx32": tr.assert_f32(got["dx32"][:m], r, bnd, label + " dx32")}
    for name in ("dg", "db"):
        shares[name] = fp.assert_within(got[name], *rb[name], f"{label}: {name}")
    print(f"SHARE {label} " + " ".join(f"{k}={v:.4f}" for k, v in shares.items()) + f" dx16_not_rne={odd}")
    return shares


def test_some_tested_shape_is_split():
    from multihop_dense_retrieval_amd import layernorm
    split = [(M, H) + layernorm.backward_chunks(M, H) for H in ref.HS for M in ms_for(H)]
    for M, H, S, rpc in split:
        assert (S, rpc) == ref.chunks(M, H)
    assert any(S > 1 for *_, S, _ in split)
    deep = [(M, S, rpc) for M, H, S, rpc in split if H == 64 and rpc >= 8 and M % rpc and S >= 3]
    assert len(deep) >= 2, split  # a wave walks several rows, the last chunk is ragged, the partial sums are reduced
    assert any(S == 1 for *_, S, _ in split)  # and the workgroup that writes dg and db itself


LARGE_HM = [pytest.param(H, M, id=f"H{H}-M{M}") for H, M in ref.LARGE_HM]


def test_large_shapes_walk_rows_and_fill_the_strands():
    """LARGE_HM against the LIBRARY's split: rows_per_chunk >= 12, a ragged last chunk, S > 16 * 16 (layernorm_grad_ref.assert_large)"""
    from multihop_dense_retrieval_amd import layernorm
    assert ref.assert_large(chunks_of=layernorm.backward_chunks) == ref.assert_large()
    S, rpc = ref.chunks(5461, 768)
    m = ref.large_ms(5461, 768)[2]
    assert (S - 2) * rpc < m < (S - 1) * rpc  # test_rows_behind_m_dev_do_not_exist: m cuts the last chunk but one, the last one lies whole behind it


@pytest.mark.parametrize("combo", ref.TRUNK_COMBOS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("family", list(ref.FAMILIES))
@pytest.mark.parametrize("H,M", LARGE_HM)
def test_families_within_the_derived_bound_at_training_row_counts(H, M, family, combo):
    """test_families_within_the_derived_bound at LARGE_HM: every family on the three trunk combinations, the unit family also under 2^8;
    one combination per case, so that a case holds one fp64 reference (two for the unit family)"""
    for scale in ((1.0, 256.0) if family == "unit" else (1.0,)):
        case = ref.make_case(family, combo, M, H, 11, scale)
        check_bound(run(**case), ref.reference_and_bound(**case), M, f"family={family} H={H} M={M} combo={'-'.join(map(str, combo))} scale={scale:g}")


@pytest.mark.parametrize("family", list(ref.FAMILIES))
@pytest.mark.parametrize("H", ref.HS)
def test_families_within_the_derived_bound(H, family):
    """Every family, the three trunk combinations at every M and every operand combination at M = 5 and 300, at unit scale and under 2^8 where
    the family stays inside fp16; at M = 300 also with a valid-row count and old values."""
    worst = {}
    for M in ms_for(H):
        for combo in combos_for(M):
            for scale in ((1.0, 256.0) if ref.FAMILIES[family] else (1.0,)):
                case = ref.make_case(family, combo, M, H, 11, scale)
                label = f"family={family} H={H} M={M} combo={'-'.join(map(str, combo))} scale={scale:g}"
                sh = check_bound(run(**case), ref.reference_and_bound(**case), M, label)
                if M == 300:
                    old_dg, old_db = fp.grid((H,), 12, 4.0), fp.grid((H,), 13, 4.0)
                    got = run(**case, m=M - 1, old_dg=old_dg, old_db=old_db, accumulate=True)
                    check_bound(got, ref.reference_and_bound(**case, m=M - 1, old_dg=old_dg, old_db=old_db), M - 1, label + " m=M-1 accumulate")
                for k, v in sh.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(f"SHARE kernel=ln_grad family={family} H={H} " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))


def grid_case(M, H, seed, combo=ref.TRUNK_COMBOS[0]):
    """a realistic x with dy16 and dy2 on the grid of multiples of 1/8"""
    case = ref.make_case("unit", combo, M, H, seed)
    if case["dy16"] is not None:
        case["dy16"] = fp.grid((M, H), seed + 1).astype(np.float16)
    if case["dy2"] is not None:
        case["dy2"] = fp.grid((M, H), seed + 2).astype(case["dy2"].dtype)
    return case


def exact_db(case, m, old=None):
    dy = sum(case[k][:m].astype(np.float64) for k in ("dy16", "dy2") if case[k] is not None)
    db = np.zeros(case["g"].shape[0]) + (dy.sum(axis=0) if m else 0.0) + (0.0 if old is None else old.astype(np.float64))
    assert (db * 8 == np.round(db * 8)).all() and np.abs(db).max() * 8 < 2 ** 24
    return db.astype(np.float32)


@pytest.mark.parametrize("H", ref.HS)
def test_db_on_the_grid_equals_the_integer_column_sums(H):
    """every shape, row count and S, with accumulate too: the chunk seams, the ragged last chunk, the wave order and the reduction without a tolerance"""
    old = fp.grid((H,), 5, 4.0)
    for M in ms_for(H):
        for combo in ref.TRUNK_COMBOS[:2] + ref.OTHER_COMBOS[:2]:
            case = grid_case(M, H, 3, combo)
            for m in sorted({None, 0, 1, M - 1, M // 2}, key=lambda v: -1 if v is None else v):
                mm = M if m is None else m
                got = run(**case, m=m)["db"]
                assert np.array_equal(bits(got), bits(exact_db(case, mm))), (M, H, combo, m, ref.chunks(M, H))
                got = run(**case, m=m, old_db=old, old_dg=old, accumulate=True)["db"]
                assert np.array_equal(got, exact_db(case, mm, old)), (M, H, combo, m, "accumulate")
                got = run(**case, m=m, old_db=old, old_dg=old, accumulate=False)["db"]
                assert np.array_equal(got, exact_db(case, mm)), (M, H, combo, m, "overwrite")


@pytest.mark.parametrize("H,M", LARGE_HM)
def test_db_on_the_grid_equals_the_integer_column_sums_at_training_row_counts(H, M):
    """test_db_on_the_grid_equals_the_integer_column_sums at LARGE_HM: the row walk of a wave, 342 to 684 chunks through the sixteen strands and
    the ragged last chunk without a tolerance; valid-row counts inside a chunk with hundreds of whole chunks, and with one, behind them"""
    old = fp.grid((H,), 5, 4.0)
    for combo in ref.TRUNK_COMBOS[:2]:
        case = grid_case(M, H, 3, combo)
        for m in (None,) + ref.large_ms(M, H)[:3]:
            mm = M if m is None else m
            got = run(**case, m=m, outs="gb")["db"]
            assert np.array_equal(bits(got), bits(exact_db(case, mm))), (M, H, combo, m, ref.chunks(M, H))
            got = run(**case, m=m, outs="gb", old_db=old, old_dg=old, accumulate=True)["db"]
            assert np.array_equal(got, exact_db(case, mm, old)), (M, H, combo, m, "accumulate")


@pytest.mark.parametrize("H", ref.HS)
def test_zero_dy_and_zero_gamma_give_exact_zeros(H):
    old_dg, old_db = fp.grid((H,), 6, 4.0) + 0.125, fp.grid((H,), 7, 4.0) + 0.125  # (no zero among them: an old -0 would not keep its sign)
    for M in (1, 5, 300) + (tuple(ref.split_ms(H)[:1]) if H == 64 else ()):
        for combo in ref.TRUNK_COMBOS:
            case = ref.make_case("unit", combo, M, H, 41)
            zero = dict(case, dy16=np.zeros_like(case["dy16"]), dy2=np.zeros_like(case["dy2"]))
            got = run(**zero)
            for k in ("dx16", "dx32", "dg", "db"):
                assert not got[k].any(), (M, H, combo, k)
            got = run(**zero, old_dg=old_dg, old_db=old_db, accumulate=True)
            assert np.array_equal(bits(got["dg"]), bits(old_dg)) and np.array_equal(bits(got["db"]), bits(old_db)), (M, H, combo)
            full = run(**case)
            got = run(**dict(case, g=np.zeros(H, np.float32)))
            assert not got["dx16"].any() and not got["dx32"].any(), (M, H, combo)
            assert np.array_equal(bits(got["dg"]), bits(full["dg"])) and np.array_equal(bits(got["db"]), bits(full["db"])), (M, H, combo)


def poison(case, m):
    """NaN and Inf in every input row at or behind m"""
    out = dict(case)
    for k in ("inp", "res", "dy16", "dy2"):
        if case[k] is not None:
            a = case[k].copy()
            a[m:] = np.nan
            a[m + 1::2] = np.inf if k != "res" else -np.inf
            out[k] = a
    return out


@pytest.mark.parametrize("combo", ref.TRUNK_COMBOS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("H,M", [(192, 9), (768, 300), (64, ref.split_ms(64)[0] + 2), (768, 5461)])
def test_rows_behind_m_dev_do_not_exist(H, M, combo):
    """m in {0, 1, M - 1, M, M + 7} (768 x 5461: layernorm_grad_ref.large_ms -- inside a chunk, with hundreds of whole chunks and with one behind
    it), rows at or behind m NaN and Inf in every input: the results are those of the call on the first m rows alone, bit for bit (the two calls cut the rows alike wherever rows_per_chunk agrees, and the chunks behind m add +0); m = 0 gives zeros, or the old
    bits with accumulate; m = M + 7 is clamped to M. dx rows at or behind m keep the sentinel (run() asserts it)."""
    case = ref.make_case("unit", combo, M, H, 17)
    old_dg, old_db = fp.grid((H,), 18, 4.0) + 0.125, fp.grid((H,), 19, 4.0) + 0.125
    full = run(**case)
    over = run(**case, m=M + 7)
    for k in full:
        assert np.array_equal(bits(over[k]), bits(full[k])), (k, "m = M + 7")
    for m in (ref.large_ms(M, H) if (H, M) in ref.LARGE_HM else (0, 1, M - 1, M)):
        got = run(**poison(case, m), m=m)
        if m == 0:
            assert not got["dg"].any() and not got["db"].any()
            acc = run(**poison(case, 0), m=0, old_dg=old_dg, old_db=old_db, accumulate=True)
            assert np.array_equal(bits(acc["dg"]), bits(old_dg)) and np.array_equal(bits(acc["db"]), bits(old_db))
            continue
        assert all(np.isfinite(got[k][:m]).all() for k in ("dx16", "dx32")) and np.isfinite(got["dg"]).all() and np.isfinite(got["db"]).all(), m
        short = {k: (None if v is None else v[:m]) if k != "g" else v for k, v in case.items()}
        alone = run(**short)
        assert np.array_equal(bits(got["dx16"][:m]), bits(alone["dx16"])) and np.array_equal(bits(got["dx32"][:m]), bits(alone["dx32"])), m
        if ref.chunks(m, H)[1] == ref.chunks(M, H)[1]:
            assert np.array_equal(bits(got["dg"]), bits(alone["dg"])) and np.array_equal(bits(got["db"]), bits(alone["db"])), m
        else:  # another cut, another summation order: the same sums inside the bound
            rb = ref.reference_and_bound(**case, m=m)
            assert fp.worst_ratio(got["dg"], *rb["dg"])[0] <= 1.0 and fp.worst_ratio(got["db"], *rb["db"])[0] <= 1.0, m
    assert ref.chunks(1, H)[1] == ref.chunks(M, H)[1] or M > 4096  # the small shapes compare dg and db bit for bit at every m


@pytest.mark.parametrize("H,M", [(192, 23), (768, 150)])
def test_nan_in_a_valid_row_reaches_only_what_it_touches(H, M):
    case = ref.make_case("unit", ref.TRUNK_COMBOS[1], M, H, 23)
    clean = run(**case)
    row, col = M // 2, 5
    bad = dict(case, dy2=case["dy2"].copy())
    bad["dy2"][row, col] = np.nan
    got = run(**bad)
    assert np.isnan(got["dx16"][row]).all() and np.isnan(got["dx32"][row]).all() and np.isnan(got["dg"][col]) and np.isnan(got["db"][col])
    rows, cols = np.arange(M) != row, np.arange(H) != col
    for k in ("dx16", "dx32"):
        assert np.array_equal(bits(got[k][rows]), bits(clean[k][rows])), k
    for k in ("dg", "db"):
        assert np.array_equal(bits(got[k][cols]), bits(clean[k][cols])), k


@pytest.mark.parametrize("H,M", [(192, 300), (768, 300), (64, ref.split_ms(64)[1]), (192, 8200)])
def test_two_runs_and_a_larger_workspace_give_the_same_bits(H, M):
    for combo in ref.TRUNK_COMBOS:
        case = ref.make_case("unit", combo, M, H, 29)
        a, b, c = run(**case), run(**case), run(**case, ws_extra=4096 + 16)
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])) and np.array_equal(bits(a[k]), bits(c[k])), (combo, k)


@pytest.mark.parametrize("H,M", [(192, 300), (1024, 300), (64, ref.split_ms(64)[0]), (1024, 4101)])
def test_permuting_the_rows_permutes_dx_and_leaves_db_on_the_grid(H, M):
    """a row's dx bits depend on that row's inputs and g only: not on where the row stands, nor on M"""
    case = grid_case(M, H, 31)
    base = run(**case)
    perm = np.random.default_rng(31).permutation(M)
    got = run(**{k: (v if k == "g" or v is None else v[perm]) for k, v in case.items()})
    for k in ("dx16", "dx32"):
        assert np.array_equal(bits(got[k]), bits(base[k][perm])), k
    assert np.array_equal(bits(got["db"]), bits(base["db"])) and np.array_equal(bits(base["db"]), bits(exact_db(case, M)))
    few = run(**{k: (v if k == "g" or v is None else v[perm][:7]) for k, v in case.items()})
    for k in ("dx16", "dx32"):
        assert np.array_equal(bits(few[k]), bits(base[k][perm][:7])), k


def test_single_outputs_match_the_full_call():
    """each output alone (the other pointers NULL) gives the bits of the call that computes all four"""
    for M, H in ((9, 192), (300, 768)):
        case = ref.make_case("unit", ref.TRUNK_COMBOS[2], M, H, 37)
        full = run(**case)
        for outs, k in (("x", "dx16"), ("X", "dx32"), ("g", "dg"), ("b", "db")):
            assert np.array_equal(bits(run(**case, outs=outs)[k]), bits(full[k])), (M, H, k)


def test_host_validation_writes_nothing():
    from multihop_dense_retrieval_amd import layernorm
    lib = layernorm.lib()
    M, H = 70, 192
    case = ref.make_case("unit", ref.TRUNK_COMBOS[0], M, H, 43)
    inp, res16, dy16, dy2, g = (dev(case[k]) for k in ("inp", "res", "dy16", "dy2", "g"))
    res32 = torch.zeros((M, H), dtype=torch.float32, device="cuda")
    dx16 = torch.full((M, H), SENTINEL, dtype=torch.float16, device="cuda")
    dx32 = torch.full((M, H), SENTINEL, dtype=torch.float32, device="cuda")
    dg = torch.full((H + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    db = torch.full((H,), SENTINEL, dtype=torch.float32, device="cuda")
    need = int(lib.mdr_layernorm_backward_workspace_bytes(M, H, 3))
    assert need > 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    cases = [
        ("NULL in", E_INVALID, dict(inp=None)), ("NULL g", E_INVALID, dict(g=None)), ("both dy NULL", E_INVALID, dict(dy16=None, dy2=None)),
        ("both residuals", E_INVALID, dict(res32=res32)), ("no outputs", E_INVALID, dict(dx16=None, dx32=None, dg=None, db=None)),
        ("M = 0", E_INVALID, dict(M=0)), ("M < 0", E_INVALID, dict(M=-3)), ("H = 0", E_INVALID, dict(H=0)), ("H = 96", E_INVALID, dict(H=96)),
        ("H = 1088", E_INVALID, dict(H=1088)), ("H < 0", E_INVALID, dict(H=-64)), ("in_f16 = 2", E_INVALID, dict(in_f16=2)),
        ("dy2_f32 = 2", E_INVALID, dict(dy2_f32=2)), ("misaligned dg", E_INVALID, dict(dg=dg[1:])), ("misaligned dy16", E_INVALID, dict(dy16=dy16.reshape(-1)[1:])),
        ("short workspace", E_WORKSPACE, dict(ws_bytes=need - 1)), ("NULL workspace", E_WORKSPACE, dict(ws=None)),
    ]
    for label, code, change in cases:
        a = dict(inp=inp, in_f16=0, res16=res16, res32=None, dy16=dy16, dy2=dy2, dy2_f32=0, M=M, m_dev=None, H=H, g=g, eps=ref.EPS, dx16=dx16, dx32=dx32,
                 dg=dg[:H], db=db, accumulate=0, ws=ws, ws_bytes=need)
        a.update(change)
        rc = raw_call(**a)
        assert rc == code, (label, rc)
        assert lib.mdr_last_error(), label
    torch.cuda.synchronize()
    assert (dx16 == SENTINEL).all() and (dx32 == SENTINEL).all() and (dg == SENTINEL).all() and (db == SENTINEL).all() and (ws == 0x5A).all(), \
        "a rejected call wrote something"
    with pytest.raises(ValueError, match=r"\[70, 192\]"):
        layernorm.layer_norm_backward(inp, res16, dy16[:, :64].contiguous(), None, g)
    with pytest.raises(ValueError):
        layernorm.layer_norm_backward(inp, res16, None, None, g)
    with pytest.raises(ValueError):
        layernorm.layer_norm_backward(inp, res16, dy16, None, g.half())
    with pytest.raises(ValueError):
        layernorm.packed_layer_norm(inp[:, :96].contiguous(), None, g[:96].contiguous(), g[:96].contiguous())
    with pytest.raises(ValueError):
        layernorm.packed_layer_norm(inp, res16, g, g, rows=torch.tensor([3], device="cuda"))  # int64


def forward_hook(inp, res, g, b, eps, m, want32):
    """mdr_test_layernorm on numpy inputs -> (float16 [M, H], float32 [M, H] or None); rows at or behind m zero"""
    from multihop_dense_retrieval_amd import _lib
    M, H = inp.shape
    o16 = torch.zeros((M, H), dtype=torch.float16, device="cuda")
    o32 = torch.zeros((M, H), dtype=torch.float32, device="cuda") if want32 else None
    m_dev = None if m is None else torch.tensor([m], dtype=torch.int32, device="cuda")
    held = [dev(a) for a in (inp, res if res is not None and res.dtype == np.float16 else None, res if res is not None and res.dtype == np.float32 else None, g, b)]
    _lib.check(_lib.lib().mdr_test_layernorm(ptr(held[0]), 1 if inp.dtype == np.float16 else 0, ptr(held[1]), ptr(held[2]), M, ptr(m_dev), H, ptr(held[3]), ptr(held[4]),
                                             eps, ptr(o16), ptr(o32), 0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    return o16.cpu().numpy(), None if o32 is None else o32.cpu().numpy()


@pytest.mark.parametrize("rows", [False, True], ids=["all-rows", "rows"])
@pytest.mark.parametrize("keep32", [False, True], ids=["y16", "keep32"])
@pytest.mark.parametrize("combo", ref.TRUNK_COMBOS + ref.OTHER_COMBOS[:1], ids=lambda c: "-".join(map(str, c[:2])))
def test_packed_layer_norm(combo, keep32, rows):
    from multihop_dense_retrieval_amd import layernorm
    M, H = 150, 768
    m = M - 3 if rows else None
    mm = M if m is None else m
    case = ref.make_case("unit", (combo[0], combo[1], True, "f32" if keep32 else None), M, H, 47)
    bias = (0.2 * np.random.default_rng(47).standard_normal(H)).astype(np.float32)
    tx = dev(case["inp"]).requires_grad_(True)
    tres = None if case["res"] is None else dev(case["res"]).requires_grad_(True)
    tw, tb = dev(case["g"]).requires_grad_(True), dev(bias).requires_grad_(True)
    trows = None if m is None else torch.tensor([m], dtype=torch.int32, device="cuda")
    out = layernorm.packed_layer_norm(tx, tres, tw, tb, ref.EPS, trows, keep32)
    y16, y32 = out if keep32 else (out, None)
    assert y16.dtype == torch.float16 and tuple(y16.shape) == (M, H) and (y32 is None or (y32.dtype == torch.float32 and tuple(y32.shape) == (M, H)))
    f16, f32 = forward_hook(case["inp"], case["res"], case["g"], bias, ref.EPS, m, keep32)
    assert np.array_equal(bits(y16.detach().cpu().numpy()), bits(f16)), "forward bits differ from the encoder's LayerNorm"
    if keep32:
        assert np.array_equal(bits(y32.detach().cpu().numpy()), bits(f32)), "forward fp32 bits differ from the encoder's LayerNorm"
    loss = (y16.float() * dev(case["dy16"]).float()).sum()  # the gradient of y16 arrives as fp16(dy16) = dy16
    if keep32:
        loss = loss + (y32 * dev(case["dy2"])).sum()
    loss.backward()
    torch.cuda.synchronize()
    rb = ref.reference_and_bound(**case, m=m)
    label = f"packed_layer_norm {combo[0]} {combo[1]} keep32={keep32} rows={rows}"
    for name, t in (("x", tx), ("residual", tres)):
        if t is None:
            continue
        assert t.grad.dtype == t.dtype and tuple(t.grad.shape) == (M, H), name
        got = t.grad.cpu().numpy()
        assert not got[mm:].any(), name
        if got.dtype == np.float16:
            tr.assert_f16(got[:mm], *rb["dx"], f"{label} d{name}")
        else:
            print(f"SHARE {label} d{name}={tr.assert_f32(got[:mm], *rb['dx'], f'{label} d{name}'):.4f}")
    assert tw.grad.dtype == torch.float32 and tb.grad.dtype == torch.float32 and tuple(tw.grad.shape) == (H,) and tuple(tb.grad.shape) == (H,)
    for name, t in (("dg", tw), ("db", tb)):
        worst, at = fp.worst_ratio(t.grad.cpu().numpy(), *rb[name])
        print(f"SHARE {label} {name}={worst:.4f}")
        assert worst <= 1.0, (label, name, worst, at)


# ---- the CLS gather's backward --------------------------------------------------------------------------------------------------------------
def cls_call(d, cu, B, H, acc):
    from multihop_dense_retrieval_amd import _lib, layernorm
    return layernorm.lib().mdr_gather_cls_backward(ptr(d), ptr(cu), B, H, ptr(acc), 0, _lib.current_stream_ptr())


@pytest.mark.parametrize("H", [64, 192, 768, 1024])
@pytest.mark.parametrize("lens", [[5], [0, 0, 3, 1, 0, 0, 7, 2, 0], [4] * 38, [0, 2, 0]], ids=["B1", "empties", "B38", "empty-ends"])
def test_gather_cls_backward_on_the_grid(lens, H):
    """row cu[b] of every non-empty sequence becomes acc + d[b], exactly (multiples of 1/8 of magnitude at most 4 are fp16 values); empty
    sequences in front, in the middle and at the end are skipped (the last ones' cu[b] is T, the first guard row); every other row and the
    guards keep their bits"""
    from multihop_dense_retrieval_amd import _lib, layernorm
    B, cu = len(lens), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    T = int(cu[-1])
    acc0 = np.full((GUARD + T + GUARD, H), SENTINEL, np.float16)
    acc0[GUARD:GUARD + T] = fp.grid((T, H), 51).astype(np.float16)
    d = fp.grid((B, H), 52).astype(np.float16)
    want = acc0.copy()
    for b in range(B):
        if lens[b] > 0:
            want[GUARD + cu[b]] = (acc0[GUARD + cu[b]].astype(np.float32) + d[b].astype(np.float32)).astype(np.float16)
    assert (want[GUARD:GUARD + T].astype(np.float64) * 8 == np.round(want[GUARD:GUARD + T].astype(np.float64) * 8)).all()
    acc, td, tcu = dev(acc0), dev(d), dev(cu)
    _lib.check(cls_call(td, tcu, B, H, acc[GUARD:]))
    torch.cuda.synchronize()
    assert np.array_equal(bits(acc.cpu().numpy()), bits(want))
    acc2 = dev(acc0[GUARD:GUARD + max(T, 1)].copy())
    assert layernorm.gather_cls_backward(td, tcu, acc2) is acc2
    torch.cuda.synchronize()
    assert np.array_equal(bits(acc2.cpu().numpy()[:T]), bits(want[GUARD:GUARD + T]))


def test_gather_cls_backward_host_validation_writes_nothing():
    from multihop_dense_retrieval_amd import layernorm
    lib = layernorm.lib()
    B, H = 3, 128
    cu = dev(np.asarray([0, 2, 4, 6], np.int32))
    d = dev(fp.grid((B, H), 53).astype(np.float16))
    acc = torch.full((6, H), SENTINEL, dtype=torch.float16, device="cuda")
    for label, change in (("NULL d", dict(d=None)), ("NULL cu", dict(cu=None)), ("NULL acc", dict(acc=None)), ("B = 0", dict(B=0)), ("B < 0", dict(B=-1)),
                          ("H = 96", dict(H=96)), ("H = 0", dict(H=0)), ("H = 1088", dict(H=1088)), ("misaligned acc", dict(acc=acc.reshape(-1)[1:])),
                          ("misaligned d", dict(d=d.reshape(-1)[1:]))):
        a = dict(d=d, cu=cu, B=B, H=H, acc=acc)
        a.update(change)
        assert cls_call(**a) == E_INVALID, label
        assert lib.mdr_last_error(), label
    torch.cuda.synchronize()
    assert (acc == SENTINEL).all(), "a rejected call wrote something"
    with pytest.raises(ValueError):
        layernorm.gather_cls_backward(d, cu[:3].contiguous(), acc)
    with pytest.raises(ValueError):
        layernorm.gather_cls_backward(d.float(), cu, acc)
