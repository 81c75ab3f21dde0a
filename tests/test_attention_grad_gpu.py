"""GPU (-m gpu): the attention backward in isolation (mdr_attention_backward, include/mdr_attention_grad.h) against the fp64 statement of
tests/attention_grad_ref.py. EVERY element of EVERY row of dQ | dK | dV is compared; nothing is averaged.

The bar is attention_grad_ref's bound, derived from the formats and the rounding points listed in csrc/mdr_attention_grad.hip and shown on the
host (tests/test_attention_grad_host.py) to hold a second implementation of the dataflow and to throw out each index / mask / scale defect. No
tolerance here was read off a device. The one-hot, zero-score and zero-gradient cases assert EQUALITY with bit-known outputs.

Many lengths are packed into one ragged call: at one head every length from 1 to 129 (twice the block of 64 owners, plus one); at twelve
heads and L = 512 the lengths -1, 0, +1 around every multiple of the MFMA tile of 16 (the owner blocks and swept chunks of 64 are multiples
of it) with 1, 2, 70, 300, 350, 511 and 512, in four interleaved groups so that a case's fp64 reference takes a few seconds; at sixteen
heads (the answer reader's, a row stride of 3072 halves) the second of those groups in two families, and the one-hot case. dqkv starts
as a finite sentinel with 64 guard rows on both sides, which must keep their bits, in every call of this file.
"""
import ctypes

import numpy as np
import pytest
import torch

import attention_grad_ref as ref
from guarded import E_INVALID, E_WORKSPACE, OK, SENTINEL, Guarded
from multihop_dense_retrieval_amd._lib import ptr
from oracle import attention_oracle as ao
from oracle import fp
from oracle.fp import bits

pytestmark = pytest.mark.gpu

GUARD = 64        # rows of dqkv in front of and behind the call's own, which must keep their bits
LENS = [pytest.param(1, 129, ref.LENS_SWEEP, id="h1-L129-sweep")] + [
    pytest.param(12, 512, ref.LENS_EDGES[g::4], id=f"h12-L512-edges{g}") for g in range(4)]
# The answer reader's ELECTRA-large: 16 heads, a row stride of 3 x 1024 halves in qkv and dqkv, where every case above has 64 or 768 per part.
# One group of the edge lengths, in the two families that carry the most (realistic rows under four times the score scale, and a spike of 16).
H16 = (16, 512, ref.LENS_EDGES[1::4])
H16_ID = "h16-L512-edges1"
H16_FAMILIES = ("realistic4", "spike16")


def with_h16(params):
    """params x every family, plus the 16-head case in H16_FAMILIES: [(heads, L, lens, family)] with the ids the stacked decorators gave"""
    out = [pytest.param(*p.values, f, id=f"{p.id}-{f}") for f in ref.FAMILY_NAMES for p in params]
    return out + [pytest.param(*H16, f, id=f"{H16_ID}-{f}") for f in H16_FAMILIES]


def call(qkv, dctx, cu, heads, L, mode, out, ws="auto", stream="current"):
    """One raw call on device tensors; returns the code."""
    from multihop_dense_retrieval_amd import _lib, attention
    lib = attention.lib()
    B, hidden = cu.numel() - 1, 64 * heads
    need = int(lib.mdr_attention_backward_workspace_bytes(B, L, heads, mode))
    w = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda") if ws == "auto" else ws
    return lib.mdr_attention_backward(ptr(qkv), ptr(dctx), ptr(cu), B, L, hidden, heads, mode, ptr(out), ptr(w), w.numel() if w is not None else 0, 0,
                                      _lib.current_stream_ptr() if stream == "current" else stream)


def run(qkv, dctx, cu, heads, L, mode=0):
    """One call. dqkv starts as SENTINEL with GUARD rows on both sides of the call's own; returns the call's rows (numpy float16) after
    asserting MDR_OK and that the guards kept their bits."""
    from multihop_dense_retrieval_amd import _lib
    lens = np.diff(np.asarray(cu, np.int64))
    assert lens.max() <= L and lens.min() >= 0  # the caller's promise
    T, hidden = int(cu[-1]), 64 * heads
    assert qkv.shape == (T, 3 * hidden) and dctx.shape == ((len(cu) - 1) if mode == 3 else T, hidden)
    dqkv = Guarded(T, (3 * hidden,), torch.float16, GUARD, GUARD)
    _lib.check(call(torch.from_numpy(qkv).cuda(), torch.from_numpy(dctx).cuda(), torch.from_numpy(np.asarray(cu, np.int32)).cuda(), heads, L, mode,
                    dqkv.own))
    torch.cuda.synchronize()
    return dqkv.checked()


def check_bound(got, qkv, dctx, cu, heads, mode, label, parts=(0, 1, 2)):
    r, bnd = ref.reference_and_bound(qkv, dctx, cu, heads, mode)
    hidden = 64 * heads
    cols = np.concatenate([np.arange(i * hidden, (i + 1) * hidden) for i in parts])

    def where(at):
        col = int(cols[at[1]])
        b = int(np.searchsorted(cu, at[0], side="right") - 1)
        return f"sequence {b}, len {int(cu[b + 1] - cu[b])}, token {at[0] - int(cu[b])}, column {col}: {'dQ dK dV'.split()[col // hidden]}, head {col % hidden // 64}"

    worst = fp.assert_within(got[:, cols], r[:, cols], bnd[:, cols], f"{label} mode {mode}", where)
    print(f"RATIO mode={mode} {label} worst |err| / bound = {worst:.4f}")
    return r, bnd


def dctx_for(cu, heads, mode, seed, scale=1.0):
    return ref.dctx_grid((len(cu) - 1) if mode == 3 else int(cu[-1]), 64 * heads, seed, scale)


@pytest.mark.parametrize("scale", [1.0, 256.0], ids=["unit", "x256"])
@pytest.mark.parametrize("heads,L,lens,family", with_h16(LENS))
def test_every_query_within_the_derived_bound(heads, L, lens, family, scale):
    qkv, cu = ao.FAMILIES[family](lens, heads, 11)
    dctx = dctx_for(cu, heads, 0, 2, scale)
    check_bound(run(qkv, dctx, cu, heads, L, 0), qkv, dctx, cu, heads, 0, f"family={family} heads={heads} L={L} scale={scale}")


@pytest.mark.parametrize("scale", [1.0, 256.0], ids=["unit", "x256"])
@pytest.mark.parametrize("heads,L,lens,family", with_h16([pytest.param(1, 129, ref.LENS_SWEEP, id="h1-L129-sweep"), pytest.param(12, 512, ref.LENS_EDGES, id="h12-L512-edges")]))
def test_first_query_within_the_derived_bound(heads, L, lens, family, scale):
    """Mode 3. The dQ rows behind a sequence's first have reference 0 and bound 0: they must compare equal to zero."""
    qkv, cu = ao.FAMILIES[family](lens, heads, 11)
    dctx = dctx_for(cu, heads, 3, 2, scale)
    check_bound(run(qkv, dctx, cu, heads, L, 3), qkv, dctx, cu, heads, 3, f"family={family} heads={heads} L={L} scale={scale}")


@pytest.mark.parametrize("heads,L,lens", [pytest.param(1, 129, ref.LENS_SWEEP, id="h1-L129-sweep"), pytest.param(12, 512, ref.LENS_EDGES[1::4], id="h12-L512-edges1"),
                                          pytest.param(*H16, id=H16_ID)])
def test_onehot_permutation_moves_dO_rows_bit_for_bit(heads, L, lens):
    """q_i = code(pi(i)): the fp16-rounded p is exactly a permutation matrix, so dV[pi(i)] == dO[i] bit for bit -- the query-to-key map of every
    tile, chunk, lane slot and block. dQ and dK stay within the bound."""
    qkv, cu, expected = ao.onehot(lens, heads, 3)
    dctx = dctx_for(cu, heads, 0, 4)
    got = run(qkv, dctx, cu, heads, L, 0)
    hidden = 64 * heads
    want = np.zeros((int(cu[-1]), hidden), np.float16)
    e = expected.astype(np.float64)
    for b, n in enumerate(lens):
        for h in range(heads):  # columns 0 and 1 of a head's V rows spell the key: pi(i) from the forward's expected output
            rows = e[int(cu[b]):int(cu[b + 1]), 64 * h:64 * h + 2]
            pi = np.rint((-rows[:, 1] * 8 - 1) * 32 + rows[:, 0] * 8 - 1).astype(np.int64)
            assert sorted(pi) == list(range(n))
            want[int(cu[b]) + pi, 64 * h:64 * h + 64] = dctx[int(cu[b]):int(cu[b + 1]), 64 * h:64 * h + 64]
    dV = got[:, 2 * hidden:]
    bad = np.argwhere(bits(dV) != bits(want))
    assert not len(bad), (len(bad), bad[0], float(dV[tuple(bad[0])]), float(want[tuple(bad[0])]))
    check_bound(got, qkv, dctx, cu, heads, 0, f"family=onehot heads={heads} L={L}", parts=(0, 1))


@pytest.mark.parametrize("mode", [0, 3])
def test_zero_scores_give_zero_dq_dk_and_bit_known_dv(mode):
    """Q = K = 0: every p is 1 / n, dQ and dK compare equal to zero; with dO on a grid and n a power of two, dV rows are the exact sum / n."""
    heads = 2
    lens = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
    seqs = []
    for n in lens:
        rng = np.random.default_rng([n, 6])
        seqs.append((np.zeros((heads, n, 64)), np.zeros((heads, n, 64)), rng.integers(-16, 17, size=(heads, n, 64)) / 8.0))
    qkv, cu = ao.pack(seqs, heads)
    dctx = dctx_for(cu, heads, mode, 5)
    got = run(qkv, dctx, cu, heads, 512, mode)
    hidden = 64 * heads
    assert (got[:, :2 * hidden] == 0).all()
    want = np.empty((int(cu[-1]), hidden), np.float16)
    for b, n in enumerate(lens):
        rows = dctx[b:b + 1] if mode == 3 else dctx[int(cu[b]):int(cu[b + 1])]
        want[int(cu[b]):int(cu[b + 1])] = (rows.astype(np.float64).sum(axis=0) / n).astype(np.float16)
    assert np.array_equal(bits(got[:, 2 * hidden:] + np.float16(0)), bits(want + np.float16(0)))  # (+ 0: -0 and +0 are one value)


@pytest.mark.parametrize("mode", [0, 3])
def test_zero_gradient_gives_zero(mode):
    lens = [1, 63, 64, 65, 300]
    qkv, cu = ao.realistic(lens, 12, 31, 1.0)
    dctx = np.zeros(((len(lens)) if mode == 3 else int(cu[-1]), 768), np.float16)
    assert (run(qkv, dctx, cu, 12, 300, mode) == 0).all()


@pytest.mark.parametrize("mode", [0, 3])
def test_two_runs_and_another_batch_order_give_the_same_bits(mode):
    """No atomics, one summation order per element: a second run repeats the bits, and a sequence's rows do not depend on where in the batch it
    stands. A sequence of length 0 is skipped."""
    heads, L = 12, 512
    lens = [300, 1, 129, 0, 512, 64, 97, 257, 33]
    qkv, cu = ao.realistic(lens, heads, 22, 1.0)
    dctx = dctx_for(cu, heads, mode, 7)
    a = run(qkv, dctx, cu, heads, L, mode)
    assert np.array_equal(bits(a), bits(run(qkv, dctx, cu, heads, L, mode)))
    perm = np.random.default_rng(5).permutation(len(lens))
    qkv2 = np.concatenate([qkv[int(cu[b]):int(cu[b + 1])] for b in perm])
    cu2 = np.concatenate([[0], np.cumsum([lens[b] for b in perm])]).astype(np.int32)
    dctx2 = dctx[perm] if mode == 3 else np.concatenate([dctx[int(cu[b]):int(cu[b + 1])] for b in perm])
    c = run(qkv2, dctx2, cu2, heads, L, mode)
    for k, b in enumerate(perm):
        assert np.array_equal(bits(c[int(cu2[k]):int(cu2[k + 1])]), bits(a[int(cu[b]):int(cu[b + 1])])), (k, b)


@pytest.mark.parametrize("mode", [0, 3])
def test_non_finite_gradients_stay_in_their_sequence(mode):
    heads, L = 12, 300
    lens = [70, 300, 129, 1, 64]
    qkv, cu = ao.realistic(lens, heads, 23, 1.0)
    dctx = dctx_for(cu, heads, mode, 8)
    clean = run(qkv, dctx, cu, heads, L, mode)
    dirty = dctx.copy()
    victim = 2
    rows = dirty[victim:victim + 1] if mode == 3 else dirty[int(cu[victim]):int(cu[victim + 1])]
    rows[0, 5], rows[0, 70], rows[-1, 700] = np.inf, np.nan, -np.inf
    got = run(qkv, dirty, cu, heads, L, mode)  # (run() asserts MDR_OK)
    for b in range(len(lens)):
        if b != victim:
            assert np.array_equal(bits(got[int(cu[b]):int(cu[b + 1])]), bits(clean[int(cu[b]):int(cu[b + 1])])), b
    assert not np.isfinite(got[int(cu[victim]):int(cu[victim + 1])].astype(np.float32)).all()
    # delivered and contained, per sequence and per head. The whole block of one head's dO in one sequence is +Inf, -Inf or NaN
    # (mode 3: the first query's row, the only one there is). Every query i of that head then has a non-finite dP_ij = dO_i . V_j and delta_i,
    # so dS_ij is non-finite for every key j -- also where P_ij has underflowed, 0 * Inf being NaN -- and with it dQ_i = sum_j dS_ij K_j,
    # dK_j = sum_i dS_ij Q_i and dV_j = sum_i P_ij dO_i: EVERY dQ, dK and dV element of that head in that sequence (mode 3: dQ of the first query;
    # the other queries' dQ rows keep the clean run's bits). The other head of the sequence and every other sequence keep their bits.
    heads, lens = 2, [1, 64, 65, 130]
    L, hidden = max(lens), 64 * heads
    qkv, cu = ao.realistic(lens, heads, 24, 1.0)
    dctx = dctx_for(cu, heads, mode, 9)
    clean = run(qkv, dctx, cu, heads, L, mode)
    assert np.isfinite(clean.astype(np.float32)).all()
    values = [np.inf, -np.inf, np.nan]
    for victim in range(len(lens)):
        lo, hi = int(cu[victim]), int(cu[victim + 1])
        for h in range(heads):
            v = values[(victim + h) % 3]
            dirty = dctx.copy()
            (dirty[victim:victim + 1] if mode == 3 else dirty[lo:hi])[:, 64 * h:64 * (h + 1)] = v
            got = run(qkv, dirty, cu, heads, L, mode)
            hit = np.zeros(got.shape, bool)
            for part in range(3):
                dq_rows = slice(lo, lo + 1) if (mode == 3 and part == 0) else slice(lo, hi)
                hit[dq_rows, part * hidden + 64 * h:part * hidden + 64 * (h + 1)] = True
            assert not np.isfinite(got[hit].astype(np.float32)).any(), (victim, h, v, "an element of the planted head stayed finite")
            assert np.array_equal(bits(got)[~hit], bits(clean)[~hit]), (victim, h, v, "the other head or another sequence changed")
    # ONE element dO[i, c] = v, head h = c // 64: dP_ij = dO_i . V_j and delta_i are non-finite for every key j, so row i of dS is -- and no other
    # row. dQ_i = sum_j dS_ij K_j: every element of dQ row i in head h. dK_j = sum_i dS_ij Q_i has that term for every j: every dK element of head
    # h in the sequence. dV_jc' = sum_i P_ij dO_ic' meets the element at c' = c alone: column c of every dV row of the sequence (P_ij = 0 gives
    # 0 * Inf = NaN). Everything else keeps the clean run's bits: a reduction that drops one non-finite partial, or a select that swallows one
    # NaN among finite terms, fails here and not above.
    for k, (victim, i, c) in enumerate([(1, 0, 3), (2, 64, 64 + 63), (3, 129, 17), (3, 70, 64), (0, 0, 100)]):
        lo, hi = int(cu[victim]), int(cu[victim + 1])
        i, h, v = (0 if mode == 3 else i), c // 64, values[k % 3]
        assert lo + i < hi
        dirty = dctx.copy()
        dirty[victim if mode == 3 else lo + i, c] = v
        got = run(qkv, dirty, cu, heads, L, mode)
        hit = np.zeros(got.shape, bool)
        hit[lo + i, 64 * h:64 * (h + 1)] = True
        hit[lo:hi, hidden + 64 * h:hidden + 64 * (h + 1)] = True
        hit[lo:hi, 2 * hidden + c] = True
        assert not np.isfinite(got[hit].astype(np.float32)).any(), (victim, i, c, v, "an element the planted one feeds stayed finite")
        assert np.array_equal(bits(got)[~hit], bits(clean)[~hit]), (victim, i, c, v, "an element the planted one does not feed changed")


def test_first_query_mode_against_every_query_mode():
    """Mode 0 fed a dctx that is zero except at rows cu[b] computes what mode 3 computes: both inside the bound of the same reference, and mode 3's
    other dQ rows compare equal to zero."""
    heads, L = 12, 350
    lens = [1, 2, 63, 64, 65, 70, 129, 300, 350]
    qkv, cu = ao.realistic(lens, heads, 24, 1.0)
    hidden = 64 * heads
    d3 = dctx_for(cu, heads, 3, 9)
    d0 = ref.dctx_first_rows(d3, cu, hidden)
    g3, g0 = run(qkv, d3, cu, heads, L, 3), run(qkv, d0, cu, heads, L, 0)
    r3, b3 = check_bound(g3, qkv, d3, cu, heads, 3, "first query, mode 3")
    worst, at = fp.worst_ratio(g0, r3, b3)  # the SAME reference and bound
    print(f"RATIO mode=0 on mode 3's reference worst |err| / bound = {worst:.4f}")
    first = np.zeros(int(cu[-1]), bool)
    first[np.asarray(cu[:-1], np.int64)] = True
    assert (g3[~first, :hidden] == 0).all()
    # mode 0 computes the other dQ rows from dO = 0: zeros as well, so the bound of 0 there holds for it too
    assert worst <= 1.0, (worst, at)


def test_bad_arguments_are_errors_without_a_launch():
    from multihop_dense_retrieval_amd import attention
    lib = attention.lib()
    qkv = torch.zeros((8, 3 * 128), dtype=torch.float16, device="cuda")
    dctx = torch.zeros((8, 128), dtype=torch.float16, device="cuda")
    cu = torch.tensor([0, 3, 8], dtype=torch.int32, device="cuda")
    out = torch.full((8, 3 * 128), SENTINEL, dtype=torch.float16, device="cuda")
    need = int(lib.mdr_attention_backward_workspace_bytes(2, 8, 2, 0))
    assert need >= 2 * 8 * 2 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(q=p(qkv), d=p(dctx), c=p(cu), B=2, L=8, hidden=128, heads=2, mode=0, o=p(out), w=p(ws), wb=need):
        return lib.mdr_attention_backward(q, d, c, B, L, hidden, heads, mode, o, w, wb, 0, None)

    for kw, word in ((dict(q=None), "NULL"), (dict(d=None), "NULL"), (dict(c=None), "NULL"), (dict(o=None), "NULL"), (dict(B=0), "B"), (dict(L=0), "L"),
                     (dict(L=513), "L"), (dict(hidden=96), "head dim"), (dict(heads=3), "head dim"), (dict(mode=1), "mode"), (dict(mode=2), "mode")):
        assert raw(**kw) == E_INVALID, kw
        assert word in lib.mdr_last_error().decode(), (kw, lib.mdr_last_error())
    for kw in (dict(wb=2 * 8 * 2 * 8 - 1), dict(w=None), dict(w=None, wb=0)):
        assert raw(**kw) == E_WORKSPACE, kw
        assert "workspace" in lib.mdr_last_error().decode()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all(), "a rejected call launched"
    assert raw() == OK and raw(mode=3, w=None, wb=0) == OK
    torch.cuda.synchronize()
    assert (out != SENTINEL).all()


@pytest.mark.parametrize("cls_only", [False, True])
def test_autograd_function_is_the_two_kernels(cls_only):
    """packed_self_attention: the forward bits are mdr_test_attention's (kernel 0, or 3 with cls_only), qkv.grad is bit-identical to a direct
    mdr_attention_backward call."""
    from multihop_dense_retrieval_amd import _lib, attention
    heads, L = 12, 300
    lens = [70, 300, 129, 1, 64]
    qkv_h, cu_h = ao.realistic(lens, heads, 25, 1.0)
    hidden = 64 * heads
    mode = 3 if cls_only else 0
    g_h = dctx_for(cu_h, heads, mode, 10)
    qkv = torch.from_numpy(qkv_h).cuda().requires_grad_(True)
    cu = torch.from_numpy(cu_h).cuda()
    g = torch.from_numpy(g_h).cuda()
    out = attention.packed_self_attention(qkv, cu, heads, L, cls_only=cls_only)
    want = torch.empty_like(out)
    _lib.check(_lib.lib().mdr_test_attention(qkv.data_ptr(), cu.data_ptr(), None, len(lens), L, hidden, heads, 3 if cls_only else 0, want.data_ptr(), 0,
                                             _lib.current_stream_ptr()))
    out.backward(g)
    torch.cuda.synchronize()
    assert out.dtype == torch.float16 and out.shape == ((len(lens) if cls_only else int(cu_h[-1])), hidden)
    assert np.array_equal(bits(out.detach().cpu().numpy()), bits(want.cpu().numpy()))
    direct = run(qkv_h, g_h, cu_h, heads, L, mode)
    assert qkv.grad.dtype == torch.float16 and np.array_equal(bits(qkv.grad.cpu().numpy()), bits(direct))
