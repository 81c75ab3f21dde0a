"""GPU (-m gpu): the embedding backward in isolation (include/mdr_embedding_grad.h) against tests/embedding_grad_ref.py: the plan against
numpy's stable argsort, the segmented sum against integer sums, the whole call against the fp64 statement, and
packed_embedding_layer_norm (multihop_dense_retrieval_amd/embedding.py) on top of it. EVERY element is compared; nothing is averaged.

Two bars. The plan is integers: EQUAL. Where the arithmetic is exact the result must be EQUAL too: the tables and dtype0 of a d on the
grid of multiples of 1/8 (any fp32 sum of a few thousand such values of magnitude at most 4 is exact in any order). Everywhere else the bar
is embedding_grad_ref's bound, derived from the formats and the rounding points listed in csrc/mdr_embedding_grad.hip and shown on the host
(tests/test_embedding_grad_host.py) to hold a second implementation of the dataflow and to throw out each defect. No tolerance here was read
off a device. Each bound check prints `SHARE ...`, the largest part of the bound the device used.

The tables are small (vocab 97, max_pos 40), so that collisions are the rule. Every float output starts as a finite sentinel (or the old
values) with guard rows behind it, the plan as ISENTINEL; tok_src / tok_pid hold ISENTINEL from `total` on, which no kernel may dereference.
Token counts: 1, 3, 4, 5 and a few hundred; and embedding_grad_ref.BL_LARGE, a batch of 150 sequences, where a wave walks three tokens of a
chunk, chunks lie behind `total` and table rows own more than the 8 pieces that the scatter sums per round (segments of up to 232 pieces).
"""
import numpy as np
import pytest
import torch

import embedding_grad_ref as ref
from guarded import E_INVALID, E_WORKSPACE, ISENTINEL, SENTINEL, Guarded, assert_untouched, dev
from multihop_dense_retrieval_amd._lib import ptr
from oracle import fp
from oracle.fp import bits

pytestmark = pytest.mark.gpu

GUARD = 8  # rows of a table / elements of a vector behind the call's own, which must keep their bits
P = ref.P


def emb():
    from multihop_dense_retrieval_amd import embedding
    return embedding


def stream():
    from multihop_dense_retrieval_amd import _lib
    return _lib.current_stream_ptr()


def check(rc):
    from multihop_dense_retrieval_amd import _lib
    _lib.check(rc)


def pack_dev(case):
    return dict(ids=dev(case["ids"]), src=dev(case["tok_src"]), pid=dev(case["tok_pid"]), total=torch.tensor([case["total"]], dtype=torch.int32, device="cuda"))


def build_plan(case, pk=None):
    """mdr_embedding_plan into a buffer of ISENTINEL -> (device plan, its words on the host)"""
    pk = pk or pack_dev(case)
    cap = len(case["tok_src"])
    nbytes = int(emb().lib().mdr_embedding_plan_bytes(cap))
    assert nbytes >= 4 * ref.plan_layout(cap)["words"]
    plan = torch.full((nbytes // 4 + GUARD,), ISENTINEL, dtype=torch.int32, device="cuda")
    check(emb().lib().mdr_embedding_plan(ptr(pk["ids"]), ptr(pk["src"]), ptr(pk["pid"]), ptr(pk["total"]), cap, case["word"].shape[0], case["pos"].shape[0],
                                         case["pad_row"], ptr(plan), nbytes, 0, stream()))
    torch.cuda.synchronize()
    words = plan.cpu().numpy()
    assert (words[ref.plan_layout(cap)["words"]:] == ISENTINEL).all(), "the plan wrote behind its layout"
    return plan, words


class Outs:
    """the float outputs of one call, each SENTINEL (or the old value) with GUARD rows / elements of SENTINEL behind it"""

    def __init__(self, case, which, old=None):
        H = case["word"].shape[1]
        self.shapes = {"dword": (case["word"].shape[0], H), "dpos": (case["pos"].shape[0], H), "dtype0": (H,), "dg": (H,), "db": (H,),
                       "d": (len(case["tok_src"]), H)}
        self.out = {k: Guarded(self.shapes[k][0], self.shapes[k][1:], torch.float32, 0, GUARD, (old or {}).get(k),
                               outside=f"{k}: the guard behind the output was written") for k in which}
        self.buf = {k: g.buf for k, g in self.out.items()}

    def ptr(self, k):
        return self.out[k].ptr() if k in self.out else None

    def host(self):
        torch.cuda.synchronize()
        return {k: g.checked() for k, g in self.out.items()}


def run_scatter(case, d32, plan, which=("dword", "dpos", "dtype0"), old=None, accumulate=False):
    cap, H = d32.shape
    o = Outs(case, which, old)
    need = int(emb().lib().mdr_embedding_scatter_workspace_bytes(cap, H))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    td = dev(d32)
    check(emb().lib().mdr_embedding_scatter(ptr(td), ptr(plan), cap, H, case["word"].shape[0], case["pos"].shape[0], o.ptr("dword"), o.ptr("dpos"), o.ptr("dtype0"),
                                            1 if accumulate else 0, ptr(ws), need, 0, stream()))
    return o.host()


def run_backward(case, plan=None, which=ref.OUTPUTS, old=None, accumulate=False, eps=ref.EPS, pk=None, ws_extra=0):
    """mdr_embedding_backward on a numpy case -> {output: float32 array}; d rows at or behind total must keep the sentinel"""
    pk = pk or pack_dev(case)
    if plan is None and ("dword" in which or "dpos" in which):
        plan = build_plan(case, pk)[0]
    cap, H = len(case["tok_src"]), case["word"].shape[1]
    o = Outs(case, which, old)
    need = int(emb().lib().mdr_embedding_backward_workspace_bytes(cap, H)) + ws_extra
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    held = [dev(case[k]) for k in ("word", "pos", "type0", "g", "dy16", "dy2")]
    check(emb().lib().mdr_embedding_backward(ptr(pk["ids"]), ptr(pk["src"]), ptr(pk["pid"]), ptr(pk["total"]), cap, ptr(held[0]), ptr(held[1]), ptr(held[2]), ptr(held[3]),
                                             H, case["word"].shape[0], case["pos"].shape[0], eps, ptr(held[4]), ptr(held[5]),
                                             1 if case["dy2"] is not None and case["dy2"].dtype == np.float32 else 0, ptr(plan), o.ptr("dword"), o.ptr("dpos"),
                                             o.ptr("dtype0"), o.ptr("dg"), o.ptr("db"), o.ptr("d"), 1 if accumulate else 0, ptr(ws), need, 0, stream()))
    got = o.host()
    if "d" in got:
        assert_untouched(got["d"][case["total"]:], "d rows at or behind total were written")
        got["d"] = got["d"][:case["total"]]
    return got


def check_bound(got, rb, label):
    shares = ref.worst_shares(got, rb)
    print(f"SHARE {label} " + " ".join(f"{k}={v:.4f}" for k, v in shares.items()))
    bad = {k: v for k, v in shares.items() if not v <= 1.0}
    assert not bad, (label, bad)
    return shares


# ---- the plan ------------------------------------------------------------------------------------------------------------------------------
PLAN_CASES = [(kind, B, L) for B, L in ref.BL_SWEEP for kind in ("random", "equal", "range", "empty", "none")] + \
             [("distinct", 2, 3), ("distinct", 7, 13), ("random", 200, 50), ("equal", 200, 50), ("range", 200, 50)]


@pytest.mark.parametrize("kind,B,L", PLAN_CASES, ids=lambda v: str(v))
def test_plan_equals_numpy_stable_argsort(kind, B, L):
    """order, segment starts, segment rows, segment counts and keys, bit for bit, with and without pad_row; masks that are no prefixes,
    empty sequences, total = 0, clamped ids, tok_pid beyond max_pos (L = 50); 200 x 50 passes several LDS tiles and scan rounds"""
    tables = ref.make_tables("unit", 64, 1)
    for pad_row in (1, -1):
        case = dict(ref.make_pack(kind, B, L, 3), **tables, pad_row=pad_row)
        if (B, L) == (200, 50):
            assert case["total"] > 4096
        if kind == "none":
            assert case["total"] == 0
        if L == 50 and kind != "none":
            assert (case["tok_pid"][:case["total"]] >= ref.MAX_POS).any()
        ref.assert_plan(build_plan(case)[1], case, f"plan {kind} B={B} L={L} pad_row={pad_row}")


# ---- the segmented sum, exactly ------------------------------------------------------------------------------------------------------------
def old_tables(case, seed):
    H = case["word"].shape[1]
    return {"dword": fp.grid(case["word"].shape, seed, 4.0), "dpos": fp.grid(case["pos"].shape, seed + 1, 4.0), "dtype0": fp.grid((H,), seed + 2, 4.0)}


def sentinel_tables(case):
    H = case["word"].shape[1]
    return {"dword": np.full(case["word"].shape, SENTINEL, np.float32), "dpos": np.full(case["pos"].shape, SENTINEL, np.float32),
            "dtype0": fp.grid((H,), 77, 4.0)}


def check_exact(case, d32, plan, label):
    exact = ref.exact_tables(case, d32)
    got = run_scatter(case, d32, plan)
    for k in exact:
        assert np.array_equal(bits(got[k]), bits(exact[k])), (label, k, "accumulate 0: integer sums, +0 elsewhere")
    old = old_tables(case, 9)
    got = run_scatter(case, d32, plan, old=old, accumulate=True)
    want = ref.exact_tables(case, d32, old)
    for k in want:
        assert np.array_equal(got[k], want[k]), (label, k, "accumulate 1")
    old = sentinel_tables(case)
    got = run_scatter(case, d32, plan, old=old, accumulate=True)
    wid, prow = ref.rows(case)
    for k, keys in (("dword", wid), ("dpos", prow)):
        untouched = np.ones(len(got[k]), bool)
        untouched[keys[keys != case["pad_row"]]] = False
        assert np.array_equal(bits(got[k][untouched]), bits(old[k][untouched])), (label, k, "rows without a segment, and pad_row, keep the sentinel")
        assert np.array_equal(got[k][~untouched], exact[k][~untouched] + np.float32(SENTINEL)), (label, k)
    for k in ("dword", "dpos", "dtype0"):  # each output alone
        assert np.array_equal(bits(run_scatter(case, d32, plan, which=(k,))[k]), bits(exact[k])), (label, k, "alone")


@pytest.mark.parametrize("H", ref.HS)
def test_scatter_on_the_grid_equals_the_integer_sums(H):
    """segments of 1, P - 1, P, P + 1, 2 P + 1 and `total` tokens, both accumulate modes, pad_row 1 and -1"""
    tables = ref.make_tables("unit", H, 2)
    counts = {3: 1, 5: P - 1, 7: P, 9: P + 1, 11: 2 * P + 1, 1: 4, 96: 5 * P + 3, 0: 2}
    for name, pk in (("lengths", ref.make_flat(counts, 5)), ("one-segment", ref.make_flat({7: 4 * P + 5}, 6)), ("one-token", ref.make_flat({2: 1}, 7)),
                     ("five", ref.make_flat({2: 3, 4: 2}, 8))):
        for pad_row in (1, -1):
            case = dict(pk, **tables, pad_row=pad_row)
            d32 = fp.grid((len(pk["tok_src"]), H), 4)
            d32[pk["total"]:] = np.nan  # rows at or behind total are never read as values
            plan, words = build_plan(case)
            ref.assert_plan(words, case, name)
            check_exact(case, d32, plan, f"{name} H={H} pad_row={pad_row}")


@pytest.mark.parametrize("H", [64, 768])
def test_scatter_rounds_on_the_grid_equal_the_integer_sums(H):
    """segments of 8 P, 8 P + 1, 16 P - 1, 16 P + 1 and 40 P + 5 tokens -- whole rounds of eight pieces, a round of one piece, a ragged last
    round, six rounds -- and one segment of 3700 tokens (232 pieces, 29 rounds), both accumulate modes, pad_row 1 and -1"""
    tables = ref.make_tables("unit", H, 2)
    counts = {3: 8 * P, 5: 8 * P + 1, 7: 16 * P - 1, 9: 16 * P + 1, 11: 40 * P + 5, 1: 4, 0: 2}
    assert ref.ROUND == 8 * P
    for name, pk in (("rounds", ref.make_flat(counts, 15)), ("one-long-segment", ref.make_flat({7: 3700}, 16))):
        for pad_row in (1, -1):
            case = dict(pk, **tables, pad_row=pad_row)
            assert ref.longest_summed_segments(case)[0] == max(counts.values() if name == "rounds" else [3700])
            d32 = fp.grid((len(pk["tok_src"]), H), 14)
            d32[pk["total"]:] = np.nan  # rows at or behind total are never read as values
            plan, words = build_plan(case)
            ref.assert_plan(words, case, name)
            check_exact(case, d32, plan, f"{name} H={H} pad_row={pad_row}")


def test_scatter_total_zero_and_real_table_height():
    """total = 0: zeros, or the old bits with accumulate. vocab = 50265, H = 64, accumulate 1 into a table of SENTINEL: the rows that own
    tokens hold sum + SENTINEL, every other row and pad_row keep their bits."""
    tables = ref.make_tables("unit", 64, 2)
    case = dict(ref.make_pack("none", 2, 3, 1), **tables, pad_row=1)
    d32 = np.full((6, 64), np.nan, np.float32)
    plan = build_plan(case)[0]
    got = run_scatter(case, d32, plan)
    assert all(not got[k].any() and not np.signbit(got[k]).any() for k in got)
    old = old_tables(case, 3)
    got = run_scatter(case, d32, plan, old=old, accumulate=True)
    assert all(np.array_equal(bits(got[k]), bits(old[k])) for k in got)

    vocab, H = 50265, 64
    rng = np.random.default_rng(9)
    ids = np.concatenate([rng.integers(0, vocab, 300), [0] * 20, [2] * 20, [1] * 7, [vocab - 1, vocab + 5, -3]]).astype(np.int64)
    total, cap = len(ids), len(ids) + 5
    pk = dict(ids=np.concatenate([rng.permutation(ids), [4] * 5]), tok_src=np.concatenate([np.arange(total), [ISENTINEL] * 5]).astype(np.int32),
              tok_pid=np.concatenate([rng.integers(0, 600, total), [ISENTINEL] * 5]).astype(np.int32), total=total)
    case = dict(pk, word=np.zeros((vocab, H), np.float32), pos=np.zeros((514, H), np.float32), pad_row=1)
    plan, words = build_plan(case)
    ref.assert_plan(words, case, "real height")
    d32 = fp.grid((cap, H), 10)
    old = {"dword": np.full((vocab, H), SENTINEL, np.float32), "dpos": np.full((514, H), SENTINEL, np.float32)}
    got = run_scatter(case, d32, plan, which=("dword", "dpos"), old=old, accumulate=True)
    exact = ref.exact_tables(case, d32, old)
    assert np.array_equal(bits(got["dword"]), bits(exact["dword"])) and np.array_equal(bits(got["dpos"]), bits(exact["dpos"]))
    assert (got["dword"][1] == SENTINEL).all() and (got["dword"] == SENTINEL).all(axis=1).sum() >= vocab - 304


def test_a_row_depends_on_its_own_tokens_in_order_only():
    """the same ids and d rows interleaved with tokens of other ids: the rows of the original ids keep their bits (d is NOT on the grid
    here: the sums round, so the order and the pieces matter)"""
    row_depends_on_its_own_tokens(90, 2 * P)


def test_a_row_depends_on_its_own_tokens_in_order_only_over_several_rounds():
    """the same with hot ids and positions that own more than 8 P tokens: the pieces of the later rounds are the same tokens in the same order"""
    row_depends_on_its_own_tokens(600, ref.ROUND)


def row_depends_on_its_own_tokens(size, least):
    H = 192
    tables = ref.make_tables("unit", H, 2)
    rng = np.random.default_rng(12)
    base_ids = rng.choice(np.asarray([3, 5, 7, 9]), size=size, p=[0.05, 0.15, 0.3, 0.5])
    n = len(base_ids)
    d_base = rng.standard_normal((n, H)).astype(np.float32)

    def flat(ids, pids, extra=3):
        total = len(ids)
        return dict(ids=np.concatenate([ids, [3] * extra]).astype(np.int64), tok_src=np.concatenate([np.arange(total), [ISENTINEL] * extra]).astype(np.int32),
                    tok_pid=np.concatenate([pids, [ISENTINEL] * extra]).astype(np.int32), total=total, **tables, pad_row=-1)

    a = flat(base_ids, np.arange(n) % 4)
    da = np.concatenate([d_base, np.full((3, H), np.nan, np.float32)])
    ga = run_scatter(a, da, build_plan(a)[0])
    m = 2 * n + 17
    where = np.sort(rng.permutation(m)[:n])  # the original tokens keep their relative order
    ids_b, pid_b = rng.integers(20, 60, m), 10 + np.arange(m) % 9
    ids_b[where], pid_b[where] = base_ids, np.arange(n) % 4
    db_ = rng.standard_normal((m + 3, H)).astype(np.float32)
    db_[where] = d_base
    b = flat(ids_b, pid_b)
    gb = run_scatter(b, db_, build_plan(b)[0])
    assert max(np.bincount(base_ids)) > least and (least <= 2 * P or min(np.bincount(np.arange(n) % 4)) > least)
    assert np.array_equal(bits(ga["dword"][[3, 5, 7, 9]]), bits(gb["dword"][[3, 5, 7, 9]]))
    assert np.array_equal(bits(ga["dpos"][:4]), bits(gb["dpos"][:4]))
    assert not np.array_equal(bits(ga["dtype0"]), bits(gb["dtype0"]))


# ---- the whole backward --------------------------------------------------------------------------------------------------------------------
def poison(case):
    """NaN and Inf in the dy rows at or behind total"""
    out = dict(case)
    for k in ("dy16", "dy2"):
        if case[k] is not None:
            a = case[k].copy()
            a[case["total"]:] = np.nan
            a[case["total"] + 1::2] = np.inf
            out[k] = a
    return out


def old_values(case, seed):
    H = case["word"].shape[1]
    return dict(old_tables(case, seed), dg=fp.grid((H,), seed + 3, 4.0), db=fp.grid((H,), seed + 4, 4.0))


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("H", ref.HS)
def test_families_within_the_derived_bound(H, family):
    """Every element of d, dword, dpos, dtype0, dg and db on every family: 1, 3, 4, 5 and a few hundred tokens, the three gradient forms
    and clamped ids at the large shape, there also with old values; NaN and Inf in the dy rows at or behind total change nothing."""
    worst = {}
    for B, L in ref.BL_SWEEP:
        big = (B, L) == (7, 50)
        for form in (ref.DY_FORMS if big else ref.DY_FORMS[2:]):
            for kind in (("random", "range") if big else ("random",)):
                case = ref.make_case(family, H, B, L, 11, kind=kind, form=form)
                label = f"family={family} H={H} B={B} L={L} {form} {kind}"
                rb = ref.reference_and_bound(case)
                got = run_backward(case)
                sh = check_bound(got, rb, label)
                bad = run_backward(poison(case))
                for k in got:
                    assert np.array_equal(bits(got[k]), bits(bad[k])), (label, k, "NaN / Inf behind total changed the result")
                if big and form == "both":
                    old = old_values(case, 12)
                    check_bound(run_backward(case, old=old, accumulate=True), ref.reference_and_bound(case, old=old), label + " accumulate")
                for k, v in sh.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(f"SHARE kernel=embedding_backward family={family} H={H} " + " ".join(f"{k}={v:.4f}" for k, v in worst.items()))


LARGE = [pytest.param(H, kind, pad_row, id=f"H{H}-{kind}") for H in ref.HS_LARGE for kind, pad_row in ref.KINDS_LARGE]


def large_case(family, H, kind, pad_row, seed):
    """a case at BL_LARGE with its properties asserted against the LIBRARY's split"""
    case = ref.make_case(family, H, *ref.BL_LARGE, seed, kind=kind, pad_row=pad_row)
    assert ref.assert_large(case, emb().backward_chunks) == ref.assert_large(case)
    return case


@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("H,kind,pad_row", LARGE)
def test_families_within_the_derived_bound_at_training_token_counts(H, kind, pad_row, family):
    """test_families_within_the_derived_bound at BL_LARGE: every element of the six outputs on every family, with a wave walking three tokens
    of a chunk, chunks behind total and segments of more than one round; NaN and Inf in the dy rows at or behind total change nothing"""
    case = large_case(family, H, kind, pad_row, 11)
    label = f"family={family} H={H} B={ref.BL_LARGE[0]} L={ref.BL_LARGE[1]} both {kind} pad_row={pad_row}"
    print(f"SEGMENTS {label} (S, rows_per_chunk, longest word, longest pos) = {ref.assert_large(case)} total = {case['total']}")
    got = run_backward(case)
    check_bound(got, ref.reference_and_bound(case), label)
    bad = run_backward(poison(case))
    for k in got:
        assert np.array_equal(bits(got[k]), bits(bad[k])), (label, k, "NaN / Inf behind total changed the result")


@pytest.mark.parametrize("H,B,L,kind,pad_row", [pytest.param(192, 7, 50, "range", 1, id="192"), pytest.param(768, 7, 50, "range", 1, id="768")] +
                         [pytest.param(H, *ref.BL_LARGE, kind, pad_row, id=f"H{H}-{kind}") for H in ref.HS_LARGE for kind, pad_row in ref.KINDS_LARGE])
def test_two_halves_agree_and_two_runs_give_the_same_bits(H, B, L, kind, pad_row):
    """the scatter alone on the d the backward wrote gives the backward's tables and dtype0; two runs, a larger workspace and each output
    alone give the same bits"""
    case = large_case("unit", H, kind, pad_row, 29) if (B, L) == ref.BL_LARGE else ref.make_case("unit", H, B, L, 29, kind=kind, pad_row=pad_row)
    pk = pack_dev(case)
    plan = build_plan(case, pk)[0]
    a, b, c = run_backward(case, plan, pk=pk), run_backward(case, plan, pk=pk), run_backward(case, plan, pk=pk, ws_extra=4096 + 16)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])) and np.array_equal(bits(a[k]), bits(c[k])), k
    d32 = np.concatenate([a["d"], np.full((len(case["tok_src"]) - case["total"], H), np.nan, np.float32)])
    s = run_scatter(case, d32, plan)
    for k in s:
        assert np.array_equal(bits(s[k]), bits(a[k])), k
    for k in ("dword", "dpos", "dtype0", "dg", "db"):  # without d32_dev the workspace holds d
        assert np.array_equal(bits(run_backward(case, plan, which=(k,), pk=pk)[k]), bits(a[k])), (k, "alone")


@pytest.mark.parametrize("H", [64, 1024])
def test_total_says_how_many_tokens_exist(H):
    """a call with cap rows and *total = m gives the bits of the call on the first m tokens alone"""
    case = ref.make_case("unit", H, 7, 50, 31)
    full = run_backward(case)
    cap = len(case["tok_src"])
    for m in (0, 1, 5, case["total"] - 1):
        cut = dict(case, total=m)
        got = run_backward(poison(cut))
        if m == 0:
            assert all(not got[k].any() for k in ("dword", "dpos", "dtype0", "dg", "db"))
            continue
        short = dict(cut, tok_src=case["tok_src"][:m + 1].copy(), tok_pid=case["tok_pid"][:m + 1].copy(),
                     dy16=case["dy16"][:m + 1], dy2=case["dy2"][:m + 1])  # cap = m + 1: the token at m exists in the buffers only
        alone = run_backward(short)
        assert ref.chunks(m + 1, H)[1] == ref.chunks(cap, H)[1]
        for k in got:
            assert np.array_equal(bits(got[k]), bits(alone[k])), (m, k)
        assert np.array_equal(bits(got["d"]), bits(full["d"][:m]))
    over = run_backward(dict(case, total=cap + 7, tok_src=np.where(case["tok_src"] < 0, 0, case["tok_src"]), tok_pid=np.where(case["tok_pid"] < 0, 0, case["tok_pid"])))
    assert over["d"].shape[0] == cap and np.isfinite(over["dword"]).all()  # (total is clamped to cap)


@pytest.mark.parametrize("H,kind,pad_row", LARGE)
def test_total_says_how_many_tokens_exist_at_training_token_counts(H, kind, pad_row):
    """The same at BL_LARGE with *total = 0, inside the first chunk, inside a chunk with whole chunks of valid tokens on either side, and one
    short: d and the tables have the bits of the call on the first m tokens alone; that call's cap = m + 1 cuts its rows otherwise
    (rows_per_chunk 4, not 12), so dtype0, dg and db are held to the derived bound of the first m tokens instead."""
    case = large_case("unit", H, kind, pad_row, 31)
    full = run_backward(case)
    S, rpc = ref.chunks(len(case["tok_src"]), H)
    for m in (0, 5, 50 * rpc + 7, case["total"] - 1):
        cut = dict(case, total=m)
        got = run_backward(poison(cut))
        if m == 0:
            assert all(not got[k].any() for k in ("dword", "dpos", "dtype0", "dg", "db"))
            continue
        short = dict(cut, tok_src=case["tok_src"][:m + 1].copy(), tok_pid=case["tok_pid"][:m + 1].copy(),
                     dy16=case["dy16"][:m + 1], dy2=case["dy2"][:m + 1])  # cap = m + 1: the token at m exists in the buffers only
        alone = run_backward(short)
        assert ref.chunks(m + 1, H)[1] != rpc and 0 < m < case["total"]
        for k in ("d", "dword", "dpos"):
            assert np.array_equal(bits(got[k]), bits(alone[k])), (m, k)
        assert np.array_equal(bits(got["d"]), bits(full["d"][:m]))
        check_bound({k: got[k] for k in ("dtype0", "dg", "db")}, {k: v for k, v in ref.reference_and_bound(cut).items() if k in ("dtype0", "dg", "db")},
                    f"total={m} H={H} {kind}")


def test_nan_in_a_valid_row_reaches_only_what_it_touches():
    H = 192
    case = ref.make_case("unit", H, 7, 50, 23, form="dy2_f32", pad_row=-1)
    clean = run_backward(case)
    row, col = case["total"] // 2, 5
    bad = dict(case, dy2=case["dy2"].copy())
    bad["dy2"][row, col] = np.nan
    got = run_backward(bad)
    wid, prow = ref.rows(case)
    assert np.isnan(got["d"][row]).all() and np.isnan(got["dword"][wid[row]]).all() and np.isnan(got["dpos"][prow[row]]).all()
    assert np.isnan(got["dtype0"]).all() and np.isnan(got["dg"][col]) and np.isnan(got["db"][col])
    others = np.arange(case["total"]) != row
    assert np.array_equal(bits(got["d"][others]), bits(clean["d"][others]))
    assert np.array_equal(bits(np.delete(got["dword"], wid[row], 0)), bits(np.delete(clean["dword"], wid[row], 0)))
    assert np.array_equal(bits(np.delete(got["dpos"], prow[row], 0)), bits(np.delete(clean["dpos"], prow[row], 0)))
    for k in ("dg", "db"):
        assert np.array_equal(bits(np.delete(got[k], col)), bits(np.delete(clean[k], col))), k


@pytest.mark.parametrize("H", [64, 192])
def test_report_bit_equality_with_the_layernorm_backward(H):
    """Reported, not required: whether d, dg and db are bit-equal to mdr_layernorm_backward on a torch-materialised x (the generic columns of
    both kernels agree at these H). Required: both are inside the bound."""
    from multihop_dense_retrieval_amd import layernorm
    case = ref.make_case("unit", H, 7, 50, 37)
    got = run_backward(case, which=("d", "dg", "db"))
    pad = np.zeros(len(case["tok_src"]) - case["total"], np.int64)  # (rows behind total are not valid anyway: row 0)
    wid, prow = (np.concatenate([r, pad]) for r in ref.rows(case))
    x = (dev(case["word"])[dev(wid)] + dev(case["pos"])[dev(prow)]) + dev(case["type0"])
    dg, db = torch.zeros(H, device="cuda"), torch.zeros(H, device="cuda")
    _, dx32, dg, db = layernorm.layer_norm_backward(x.contiguous(), None, dev(case["dy16"]), dev(case["dy2"]), dev(case["g"]), ref.EPS,
                                                    torch.tensor([case["total"]], dtype=torch.int32, device="cuda"), False, True, dg, db)
    torch.cuda.synchronize()
    theirs = {"d": dx32.cpu().numpy()[:case["total"]], "dg": dg.cpu().numpy(), "db": db.cpu().numpy()}
    rb = ref.reference_and_bound(case)
    assert max(ref.worst_shares(theirs, rb).values()) <= 1.0
    print(f"BITEQ H={H} " + " ".join(f"{k}={np.array_equal(bits(got[k]), bits(theirs[k]))}" for k in theirs))


# ---- the autograd function -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep32", [False, True], ids=["y16", "keep32"])
def test_packed_embedding_layer_norm(keep32):
    from multihop_dense_retrieval_amd import _lib
    H = 768
    case = ref.make_case("unit", H, 7, 50, 47, kind="range", form="both" if keep32 else "dy16")
    cap, total = len(case["tok_src"]), case["total"]
    bias = (0.2 * np.random.default_rng(47).standard_normal(H)).astype(np.float32)
    pk = pack_dev(case)
    params = [dev(case[k]).requires_grad_(True) for k in ("word", "pos", "type0", "g")] + [dev(bias).requires_grad_(True)]
    out = emb().packed_embedding_layer_norm(pk["ids"], pk["src"], pk["pid"], pk["total"], *params, ref.EPS, cap, case["pad_row"], keep32)
    y16, y32 = out if keep32 else (out, None)
    f16 = torch.zeros((cap, H), dtype=torch.float16, device="cuda")
    f32 = torch.zeros((cap, H), dtype=torch.float32, device="cuda")
    check(_lib.lib().mdr_test_embed_ln(0, ptr(pk["ids"]), None, ptr(pk["src"]), ptr(pk["pid"]), ptr(pk["total"]), cap, 0, ptr(params[0]), ptr(params[1]), ptr(params[2]), 1,
                                       ptr(params[3]), ptr(params[4]), H, ref.VOCAB, ref.MAX_POS, ref.EPS, ptr(f16), ptr(f32), 0, stream()))
    assert y16.dtype == torch.float16 and torch.equal(y16.detach().view(torch.int16), f16.view(torch.int16)), "forward bits differ from the encoder's"
    if keep32:
        assert torch.equal(y32.detach().view(torch.int32), f32.view(torch.int32)), "forward fp32 bits differ from the encoder's"
    loss = (y16.float() * dev(case["dy16"]).float()).sum()  # the gradient of y16 arrives as fp16(dy16) = dy16
    if keep32:
        loss = loss + (y32 * dev(case["dy2"])).sum()
    loss.backward()
    direct = run_backward(case, which=("dword", "dpos", "dtype0", "dg", "db"))
    for k, t in zip(("dword", "dpos", "dtype0", "dg", "db"), params):
        assert t.grad.dtype == torch.float32 and t.grad.shape == t.shape, k
        assert np.array_equal(bits(t.grad.cpu().numpy()), bits(direct[k])), (k, "backward() differs from the direct call")
    check_bound({k: t.grad.cpu().numpy() for k, t in zip(("dword", "dpos", "dtype0", "dg", "db"), params)}, ref.reference_and_bound(case),
                f"packed_embedding_layer_norm keep32={keep32}")


# ---- host validation -------------------------------------------------------------------------------------------------------------------------
def test_host_validation_writes_nothing():
    lib = emb().lib()
    H = 192
    case = ref.make_case("unit", H, 7, 50, 43)
    cap = len(case["tok_src"])
    pk = pack_dev(case)
    plan_bytes = int(lib.mdr_embedding_plan_bytes(cap))
    plan = torch.full((plan_bytes // 4,), ISENTINEL, dtype=torch.int32, device="cuda")
    base = dict(ids=pk["ids"], src=pk["src"], pid=pk["pid"], total=pk["total"], cap=cap, vocab=ref.VOCAB, max_pos=ref.MAX_POS, pad_row=1, plan=plan, nbytes=plan_bytes)
    for label, code, change in [("NULL ids", E_INVALID, dict(ids=None)), ("NULL tok_src", E_INVALID, dict(src=None)), ("NULL tok_pid", E_INVALID, dict(pid=None)),
                                ("NULL total", E_INVALID, dict(total=None)), ("cap = 0", E_INVALID, dict(cap=0)), ("cap > 2^20", E_INVALID, dict(cap=2 ** 20 + 1)),
                                ("vocab = 0", E_INVALID, dict(vocab=0)), ("vocab > 2^20", E_INVALID, dict(vocab=2 ** 20 + 1)), ("max_pos = 0", E_INVALID, dict(max_pos=0)),
                                ("max_pos > 2^16", E_INVALID, dict(max_pos=2 ** 16 + 1)), ("pad_row = -2", E_INVALID, dict(pad_row=-2)),
                                ("misaligned plan", E_INVALID, dict(plan=plan[1:])), ("NULL plan", E_WORKSPACE, dict(plan=None)),
                                ("short plan", E_WORKSPACE, dict(nbytes=4 * ref.plan_layout(cap)["words"] - 1))]:
        a = dict(base, **change)
        rc = lib.mdr_embedding_plan(ptr(a["ids"]), ptr(a["src"]), ptr(a["pid"]), ptr(a["total"]), a["cap"], a["vocab"], a["max_pos"], a["pad_row"], ptr(a["plan"]),
                                    a["nbytes"], 0, stream())
        assert rc == code and lib.mdr_last_error(), (label, rc)
    torch.cuda.synchronize()
    assert (plan == ISENTINEL).all(), "a rejected plan call wrote something"
    plan = build_plan(case, pk)[0]

    o = Outs(case, ref.OUTPUTS)
    d32 = dev(fp.grid((cap, H), 1))
    sneed = int(lib.mdr_embedding_scatter_workspace_bytes(cap, H))
    bneed = int(lib.mdr_embedding_backward_workspace_bytes(cap, H))
    ws = torch.full((bneed,), 0x5A, dtype=torch.uint8, device="cuda")
    sbase = dict(d32=d32, plan=plan, cap=cap, H=H, vocab=ref.VOCAB, max_pos=ref.MAX_POS, dword=o.buf["dword"], dpos=o.buf["dpos"], dtype0=o.buf["dtype0"],
                 accumulate=0, ws=ws, nbytes=sneed)
    for label, code, change in [("NULL d32", E_INVALID, dict(d32=None)), ("NULL plan", E_INVALID, dict(plan=None)),
                                ("no outputs", E_INVALID, dict(dword=None, dpos=None, dtype0=None)), ("accumulate = 2", E_INVALID, dict(accumulate=2)),
                                ("cap = 0", E_INVALID, dict(cap=0)), ("H = 96", E_INVALID, dict(H=96)), ("H = 1088", E_INVALID, dict(H=1088)), ("H = 0", E_INVALID, dict(H=0)),
                                ("vocab = 0", E_INVALID, dict(vocab=0)), ("max_pos = 0", E_INVALID, dict(max_pos=0)),
                                ("misaligned dword", E_INVALID, dict(dword=o.buf["dword"].reshape(-1)[1:])), ("misaligned d32", E_INVALID, dict(d32=d32.reshape(-1)[1:])),
                                ("short workspace", E_WORKSPACE, dict(nbytes=ref.chunks(cap, H)[0] * H * 4 - 1)), ("NULL workspace", E_WORKSPACE, dict(ws=None))]:
        a = dict(sbase, **change)
        rc = lib.mdr_embedding_scatter(ptr(a["d32"]), ptr(a["plan"]), a["cap"], a["H"], a["vocab"], a["max_pos"], ptr(a["dword"]), ptr(a["dpos"]), ptr(a["dtype0"]),
                                       a["accumulate"], ptr(a["ws"]), a["nbytes"], 0, stream())
        assert rc == code and lib.mdr_last_error(), (label, rc)

    held = {k: dev(case[k]) for k in ("word", "pos", "type0", "g", "dy16", "dy2")}
    bbase = dict(pk, cap=cap, **held, H=H, vocab=ref.VOCAB, max_pos=ref.MAX_POS, dy2_f32=1, plan=plan, dword=o.buf["dword"], dpos=o.buf["dpos"],
                 dtype0=o.buf["dtype0"], dg=o.buf["dg"], db=o.buf["db"], d=o.buf["d"], accumulate=0, ws=ws, nbytes=bneed)
    none_out = dict(dword=None, dpos=None, dtype0=None, dg=None, db=None, d=None)
    for label, code, change in [("NULL ids", E_INVALID, dict(ids=None)), ("NULL total", E_INVALID, dict(total=None)), ("NULL word", E_INVALID, dict(word=None)),
                                ("NULL pos", E_INVALID, dict(pos=None)), ("NULL type0", E_INVALID, dict(type0=None)), ("NULL g", E_INVALID, dict(g=None)),
                                ("both dy NULL", E_INVALID, dict(dy16=None, dy2=None)), ("no outputs", E_INVALID, none_out),
                                ("tables without a plan", E_INVALID, dict(plan=None)), ("dy2_f32 = 2", E_INVALID, dict(dy2_f32=2)),
                                ("accumulate = -1", E_INVALID, dict(accumulate=-1)), ("cap = 0", E_INVALID, dict(cap=0)), ("H = 96", E_INVALID, dict(H=96)),
                                ("H = -64", E_INVALID, dict(H=-64)), ("vocab > 2^20", E_INVALID, dict(vocab=2 ** 20 + 1)), ("max_pos = 0", E_INVALID, dict(max_pos=0)),
                                ("misaligned dg", E_INVALID, dict(dg=o.buf["dg"][1:])), ("misaligned dy16", E_INVALID, dict(dy16=held["dy16"].reshape(-1)[1:])),
                                ("short workspace", E_WORKSPACE, dict(nbytes=cap * H * 4)), ("NULL workspace", E_WORKSPACE, dict(ws=None))]:
        a = dict(bbase, **change)
        rc = lib.mdr_embedding_backward(ptr(a["ids"]), ptr(a["src"]), ptr(a["pid"]), ptr(a["total"]), a["cap"], ptr(a["word"]), ptr(a["pos"]), ptr(a["type0"]), ptr(a["g"]),
                                        a["H"], a["vocab"], a["max_pos"], ref.EPS, ptr(a["dy16"]), ptr(a["dy2"]), a["dy2_f32"], ptr(a["plan"]), ptr(a["dword"]),
                                        ptr(a["dpos"]), ptr(a["dtype0"]), ptr(a["dg"]), ptr(a["db"]), ptr(a["d"]), a["accumulate"], ptr(a["ws"]), a["nbytes"], 0, stream())
        assert rc == code and lib.mdr_last_error(), (label, rc)
    torch.cuda.synchronize()
    assert all((b == SENTINEL).all() for b in o.buf.values()) and (ws == 0x5A).all(), "a rejected call wrote something"

    E = emb()
    with pytest.raises(ValueError, match=r"\[350, 192\]"):
        E.embedding_backward(pk["ids"], pk["src"], pk["pid"], pk["total"], cap, held["word"], held["pos"], held["type0"], held["g"], ref.EPS,
                             held["dy16"][:, :64].contiguous(), None, plan, dg=torch.zeros(H, device="cuda"))
    with pytest.raises(ValueError):
        E.embedding_backward(pk["ids"], pk["src"], pk["pid"], pk["total"], cap, held["word"], held["pos"], held["type0"], held["g"], ref.EPS, None, None, plan,
                             dg=torch.zeros(H, device="cuda"))
    with pytest.raises(ValueError):
        E.embedding_backward(pk["ids"], pk["src"], pk["pid"], pk["total"], cap, held["word"], held["pos"], held["type0"], held["g"], ref.EPS, held["dy16"], None,
                             plan[:10], dword=torch.zeros(ref.VOCAB, H, device="cuda"))
    with pytest.raises(ValueError):
        E.embedding_plan(pk["ids"], pk["src"].long(), pk["pid"], pk["total"], cap, ref.VOCAB, ref.MAX_POS, 1)
    with pytest.raises(ValueError):
        E.embedding_plan(pk["ids"], pk["src"], pk["pid"], pk["total"], cap, ref.VOCAB, ref.MAX_POS, -2)
    with pytest.raises(ValueError):
        E.embedding_scatter(d32, plan, ref.VOCAB, ref.MAX_POS)
    with pytest.raises(ValueError):
        E.packed_embedding_layer_norm(pk["ids"], pk["src"], pk["pid"], pk["total"], held["word"][:, :96].contiguous(), held["pos"], held["type0"], held["g"],
                                      held["g"], ref.EPS, cap, 1)
